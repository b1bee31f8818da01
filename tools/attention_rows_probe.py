#!/usr/bin/env python3
"""Time dinox_attention_rows at the two shapes the monitor meets and price it against its byte model.

    python tools/attention_rows_probe.py [--iters 200]

Shapes: ViT-S/16 at 224 (B = 32, N = 201, 6 heads x 64) and ViT-L/14 at 518 (B = 1 and B = 8, N = 1374, 16 heads x 64), bf16 and fp32,
Q = 1 (CLS) and Q = 5 (CLS + 4 registers).  Time: HIP events around `iters` back-to-back launches after a warm-up (the operand stays
in the memory-side cache between launches at these sizes, so this is the kernel on a warm cache, not a cold HBM read).  Bytes: K once
(B N heads d elements) plus the output once (B heads Q N floats) -- the model of csrc/attention_rows.hip.  One line per case.
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


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("this engine computes on MI355X only: no CUDA/HIP device available")
    from dinox import ops
    g = torch.Generator().manual_seed(0)
    shapes = [("vit-s/16@224", 32, 201, 6, 64), ("vit-l/14@518", 1, 1374, 16, 64), ("vit-l/14@518", 8, 1374, 16, 64)]
    for name, B, N, heads, d in shapes:
        for dtype in (torch.bfloat16, torch.float32):
            qkv = torch.randn(B, N, 3 * heads * d, generator=g).to(dtype).cuda()
            for idx in ((0,), (0, N - 4, N - 3, N - 2, N - 1)):
                for _ in range(10):
                    ops.attention_rows(qkv, heads, idx)
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.iters):
                    ops.attention_rows(qkv, heads, idx)
                b.record()
                torch.cuda.synchronize()
                us = a.elapsed_time(b) * 1e3 / args.iters
                nbytes = B * N * heads * d * qkv.element_size() + B * heads * len(idx) * N * 4
                print(f"attention_rows {name} B={B} N={N} heads={heads} d={d} {str(dtype).split('.')[-1]} Q={len(idx)}: "
                      f"{us:8.1f} us per call (host launch included)  model {nbytes / 1e6:7.2f} MB  {nbytes / us / 1e3:7.1f} GB/s  "
                      f"workgroups {B * heads}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
