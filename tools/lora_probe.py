#!/usr/bin/env python3
"""What a LoRA-wrapped linear layer costs: forward + backward of the four layer shapes of a ViT-S block (width 384) at M = 32 x 201 and
256 x 201 token rows, bf16 mode, for
    linear_frozen     ops.LinearFn, base frozen (dX only)
    linear_trainable  ops.LinearFn, base trainable (dX, dW, db)
    lora_r8           ops.LoraLinearFn at r = 8, base frozen (dX, dA, dB)
and dinox_lora_grad alone against the dW product (ops.weight_grad) it stands in for.  A stand-alone autograd node is issued more slowly
than the device runs it, so every timed window is DEVICE time: the stream is first held busy by a spin kernel (torch.cuda._sleep) while
the host enqueues `--batch` calls between two HIP events; the figure is the window / batch, median of `--repeats` windows after
`--warmup` untimed calls.  (Measured: the single-launch cases then follow the device; the whole-layer autograd cases still come out the
same at every shape, i.e. they remain bound by how fast a node is issued -- take a layer's device cost from the kernel trace of
`--lora-only`, as DESIGN.md does.)  Every case is measured twice in an A/A pair (the second pass after all other cases), and the larger
relative difference of such a pair is printed as the spread below which two figures here are not distinguishable.
    python tools/lora_probe.py [--out FILE.json]
    rocprofv3 --pmc FETCH_SIZE --output-format csv -d OUT -- python tools/lora_probe.py --grad-only --calls 5     (then WRITE_SIZE;
    tools/pmc_raw.py sums the counters per kernel; compare with the M (K + N) operand bytes printed by --grad-only)"""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--rank", type=int, default=8)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--batch", type=int, default=8, help="calls per timed window")
ap.add_argument("--hold-ms", type=float, default=30.0, help="how long the spin kernel holds the stream while a window is enqueued")
ap.add_argument("--grad-only", action="store_true", help="only launch dinox_lora_grad (a workload for a counter pass)")
ap.add_argument("--lora-only", metavar="LAYER", help="only run the LoRA layer of that shape (qkv, proj, fc1, fc2) at M = 256 x 201 (for a kernel trace)")
ap.add_argument("--calls", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dino-x_amd")]
import torch  # noqa: E402
from dinox import ops  # noqa: E402

DEV = "cuda"
SHAPES = {"qkv": (384, 1152), "proj": (384, 384), "fc1": (384, 1536), "fc2": (1536, 384)}
ROWS = (32 * 201, 256 * 201)
r = args.rank
gen = torch.Generator(device=DEV).manual_seed(0)



def _hold_cycles():
    """torch.cuda._sleep counts a device clock whose rate differs by platform: measure it once."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(1000)
    torch.cuda.synchronize()
    a.record()
    torch.cuda._sleep(2_000_000)
    b.record()
    b.synchronize()
    return int(args.hold_ms / max(a.elapsed_time(b), 1e-3) * 2_000_000)


HOLD_CYCLES = _hold_cycles()


def rand(*shape, scale=1.0, dtype=torch.float32):
    return (torch.randn(*shape, device=DEV, generator=gen) * scale).to(dtype)


def timed(fn):
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(HOLD_CYCLES)              # the host runs ahead of the device for the whole window
        a.record()
        for _ in range(args.batch):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / args.batch)
    ts.sort()
    return ts[len(ts) // 2]


if args.grad_only:
    M, (K, N) = ROWS[1], SHAPES["qkv"]
    xl, dy = rand(M, K, dtype=torch.bfloat16), rand(M, N, dtype=torch.bfloat16)
    A, B = rand(r, K, scale=0.05), rand(N, r, scale=0.05)
    for _ in range(args.calls):
        ops.lora_grad(xl, dy, A, B, 2.0)
    torch.cuda.synchronize()
    print(json.dumps({"calls": args.calls, "M": M, "K": K, "N": N, "r": r, "operand_bytes": M * (K + N) * 2,
                      "partials_bytes": ((M + 127) // 128) * (r * K + N * r) * 4}))
    sys.exit(0)

if args.lora_only:
    M, (K, N) = ROWS[1], SHAPES[args.lora_only]
    x, dy = rand(M, K).requires_grad_(True), rand(M, N)
    W, b = rand(N, K, scale=K ** -0.5), rand(N, scale=0.1)
    A, B = rand(r, K, scale=0.05).requires_grad_(True), rand(N, r, scale=0.05).requires_grad_(True)
    res = rand(M, N) if args.lora_only in ("proj", "fc2") else None
    with ops.compute_dtype(torch.bfloat16):
        for _ in range(args.calls):
            ops.lora_linear(x, W, b, A, B, 2.0, 0.0, None, res).backward(dy if res is not None else dy.bfloat16())
    torch.cuda.synchronize()
    print(f"lora_probe: {args.calls} forward + backward passes of the LoRA {args.lora_only} layer at M = {M}")
    sys.exit(0)

cases = {}
with ops.compute_dtype(torch.bfloat16):
    for M in ROWS:
        for name, (K, N) in SHAPES.items():
            x = rand(M, K).requires_grad_(True)
            dy = rand(M, N)
            W, b = rand(N, K, scale=K ** -0.5), rand(N, scale=0.1)
            Wt, bt = W.clone().requires_grad_(True), b.clone().requires_grad_(True)
            A, B = rand(r, K, scale=0.05).requires_grad_(True), rand(N, r, scale=0.05).requires_grad_(True)
            res = rand(M, N) if name in ("proj", "fc2") else None
            dyo = dy if res is not None else dy.bfloat16()

            def linear_frozen():
                ops.LinearFn.apply(x, W, b, res, None).backward(dyo)

            def linear_trainable():
                ops.LinearFn.apply(x, Wt, bt, res, None).backward(dyo)

            def lora():
                ops.lora_linear(x, W, b, A, B, 2.0, 0.0, None, res).backward(dyo)

            xl, dyl = x.detach().bfloat16(), dy.bfloat16()
            cases[(M, name)] = {"linear_frozen": linear_frozen, "linear_trainable": linear_trainable, f"lora_r{r}": lora,
                                "lora_grad_alone": lambda xl=xl, dyl=dyl, A=A, B=B: ops.lora_grad(xl, dyl, A, B, 2.0),
                                "weight_grad_alone": lambda xl=xl, dyl=dyl, Wt=Wt, bt=bt: ops.gemm(dyl, xl, transA=True, transB=True,
                                                                                                  out_dtype=torch.float32)}
    first = {k: {n: timed(f) for n, f in fns.items()} for k, fns in cases.items()}
    second = {k: {n: timed(f) for n, f in fns.items()} for k, fns in cases.items()}

spread = max(abs(first[k][n] - second[k][n]) / min(first[k][n], second[k][n]) for k in first for n in first[k])
out = {"rank": r, "unit": "us of device time per call, median of %d windows of %d calls" % (args.repeats, args.batch), "aa_spread": round(spread, 4), "shapes": {}}
for (M, name), t in first.items():
    row = {n: round(min(v, second[(M, name)][n]), 1) for n, v in t.items()}
    row["lora_cheaper_than_trainable_base"] = row[f"lora_r{r}"] < row["linear_trainable"]
    out["shapes"][f"M={M} {name} {SHAPES[name][0]}->{SHAPES[name][1]}"] = row
text = json.dumps(out, indent=1)
print(text)
if args.out:
    open(args.out, "w").write(text + "\n")
