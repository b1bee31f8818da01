#!/usr/bin/env python3
"""The SimCLR step at the headline shape (ViT-S/16, 224 px, batch 256, bf16, out_dim 8192):
  (a) ms/step and samples/s of TrainEngine(loss_type="simclr"), next to the dino step of the same model;
  (b) the NT-Xent head alone on a [512, out_dim] fp32 head output: normalise, two exact-fp32 products, three kernels
      (ops.ntxent_fwd + ops.ntxent_bwd), and its pieces;
  (c) the same loss and backward composed from stock PyTorch ops (F.normalize, matmul, masked_fill, cross_entropy, autograd) on the
      same device and the same tensor.
Every timed window ends in a device synchronise; windows alternate between the variants; median [min .. max] over the windows.
--quick: fewer windows and a smaller batch (a profiler's run)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dino-x_amd")]
import numpy as np, torch
import torch.nn.functional as F
import zoo.arch as arch
from dinox import ops
from dinox.engine import StepHyperParams, TrainEngine

QUICK = "--quick" in sys.argv
B, OUT, WINDOWS, REPS = (64, 8192, 3, 3) if QUICK else (256, 8192, 7, 5)
DEV = "cuda"


def window(fn, reps):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(reps): fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def spread(ts, unit=1e3, name="ms"):
    return f"{np.median(ts)*unit:.3f} {name} [{min(ts)*unit:.3f} .. {max(ts)*unit:.3f}]"


# ---- (a) the whole step
g = torch.Generator().manual_seed(0)
batch = torch.randn(2 * B, 3, 224, 224, generator=g).to(DEV)
sp = (torch.rand(B, 3, generator=g) * 2 + 0.4).repeat(2, 1).to(DEV)
kw = dict(img_size=224, patch=16, dim=384, depth=12, heads=6, num_registers=4, scale_aware=True)
engines = {}
for loss_type in ("simclr", "dino"):
    torch.manual_seed(1)
    s_ = arch.DinoStudentTeacher(arch.PatchViT(**kw), OUT)
    t_ = arch.DinoStudentTeacher(arch.PatchViT(**kw), OUT)
    t_.load_state_dict(s_.state_dict())
    engines[loss_type] = TrainEngine(s_.to(DEV), t_.to(DEV), OUT, StepHyperParams(lr=1e-4, warmup_steps=10, loss_type=loss_type),
                                     amp_dtype=torch.bfloat16)
    for _ in range(3): engines[loss_type].step(batch, sp)
times = {k: [] for k in engines}
for _ in range(WINDOWS):
    for k, eng in engines.items():
        times[k].append(window(lambda: eng.step(batch, sp), REPS))
for k, ts in times.items():
    print(f"(a) {k} step, ViT-S/16 224 bs {B} bf16 out_dim {OUT}: {spread(ts)} = {B/np.median(ts):.0f} samples/s  "
          f"(loss {engines[k].scalars()['loss']:.4f})")
del engines
torch.cuda.empty_cache()

# ---- (b) the NT-Xent head alone, (c) stock PyTorch ops on the same tensor
M = 2 * B
z = (torch.randn(M, OUT, generator=g) * 2).to(DEV)


def head_hip():
    loss, saved = ops.ntxent_fwd(z, 0.1)
    return loss, ops.ntxent_bwd(saved, 1.0)


def head_torch():
    zz = z.detach().requires_grad_(True)
    f = F.normalize(zz, dim=1)
    sim = torch.matmul(f, f.T) / 0.1
    sim = sim.masked_fill(torch.eye(M, device=DEV).bool(), -9e15)
    target = torch.cat([torch.arange(B, M, device=DEV), torch.arange(0, B, device=DEV)])
    loss = F.cross_entropy(sim, target)
    loss.backward()
    return loss.detach(), zz.grad


def head_torch_amp():          # what the reference's --amp runs: the similarity matmul autocast to bf16
    with torch.autocast("cuda", dtype=torch.bfloat16):
        return head_torch()


la, ga = head_hip(); lb, gb = head_torch()
print(f"    HIP head vs stock ops: loss {float(la):.6f} vs {float(lb):.6f}, max |dz| difference {float((ga - gb).abs().max()):.2e} "
      f"of max |dz| {float(gb.abs().max()):.2e}")
variants = {"(b) NT-Xent head, HIP kernels (fp32)": head_hip, "(c) stock PyTorch ops, fp32": head_torch,
            "(c') stock PyTorch ops, bf16 autocast": head_torch_amp}
for fn in variants.values():
    for _ in range(3): fn()
times = {k: [] for k in variants}
for _ in range(WINDOWS):
    for k, fn in variants.items():
        times[k].append(window(fn, 20))
for k, ts in times.items():
    print(f"{k}, [{M}, {OUT}]: {spread(ts, 1e6, 'us')}")

# ---- the pieces of (b), each in its own windows (launch + run; the products dominate if the expectation holds)
loss, saved = ops.ntxent_fwd(z, 0.1)
S, zh, norm, lse, inv_tau = saved
W = torch.empty_like(S)
dzh = ops.gemm(W, zh, transB=True, out_dtype=torch.float32)
f = lambda *sh: torch.empty(sh, dtype=torch.float32, device=DEV)
row_loss, l1, dz, sq = f(M), f(1), f(M, OUT), f(M)
st = torch.cuda.current_stream().cuda_stream
lib, p = ops.lib, lambda t: t.data_ptr()
pieces = {
    "normalise (dinox_koleo_normalize)": lambda: lib.dinox_koleo_normalize(p(z), p(zh), p(norm), p(sq), M, OUT, 1e-12, st),
    "S = Zh Zh^T (exact fp32, split-K)": lambda: ops.gemm_nt_f32_splitk(zh, zh),
    "ntxent_rows (+ mean)": lambda: lib.dinox_ntxent_rows(p(S), M, M, inv_tau, p(lse), p(row_loss), p(l1), st),
    "ntxent_coeff": lambda: lib.dinox_ntxent_coeff(p(S), M, p(lse), M, inv_tau, 1.0, p(W), M, st),
    "dZh = W Zh (exact fp32)": lambda: ops.gemm(W, zh, transB=True, out_dtype=torch.float32),
    "normalize_bwd": lambda: lib.dinox_normalize_bwd(p(dzh), p(zh), p(norm), p(dz), M, OUT, 1e-12, st),
}
for k, fn in pieces.items():
    for _ in range(3): fn()
    ts = [window(fn, 50) for _ in range(3 if QUICK else 5)]
    print(f"    {k}: {spread(ts, 1e6, 'us')}")
