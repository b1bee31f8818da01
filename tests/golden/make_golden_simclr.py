#!/usr/bin/env python3
"""Generate the SimCLR fixtures in this directory FROM THE REAL REFERENCE (same arrangement as make_golden.py: the reference
checkout is imported by path, runs on the CPU in fp32 with seeded inputs, and only data is written).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_simclr.py        (DINOX_REFERENCE: the reference checkout)

Fixtures
  simclr_loss.npz       SimCLRLoss(temperature=0.1) (phase5_big_run.py:776-813) + autograd on four cases: B x D = 3 x 5, 33 x 130,
                        130 x 257 (seeded normal rows) and an 8 x 16 adversarial case -- a duplicated pair, a row scaled by 1e-20
                        (below F.normalize's eps), a row scaled by 1e4, two parallel rows, an anti-parallel positive, an all-zero row
                        (logits at +1/tau and -1/tau).  Per case: z1, z2, loss
                        (float64 of the fp32 result), dz1, dz2.
  simclr_step_tiny.npz  three steps of the reference loop order with loss_type="simclr" (:1692-1700, :1728-1737, :1769-1802: no
                        teacher forward, no EMA) on the 28/14/32/2/2 scale-aware model of step_tiny, batches of 4 samples: init state,
                        batches, spacings, per-step loss / grad-norm / lr, EVERY parameter gradient of each step, the student after
                        step 3, and the share of student elements whose gradient is below 1e-6 in any step (asserted <= 10 %).
                        The initial weights and the batches are rounded to fp16-representable values BEFORE the run and stored as
                        float16 (exact): that keeps the file under the repository's 1 MiB limit without losing a bit.
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

REF = os.environ.get("DINOX_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))

sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(REF, "scripts"))
for name in ("torchvision", "torchvision.transforms"):
    sys.modules.setdefault(name, types.ModuleType(name))

import zoo.arch as A            # noqa: E402  (the reference)
import phase5_big_run as P      # noqa: E402  (the reference)

torch.set_num_threads(4)
torch.use_deterministic_algorithms(True)

TEMPERATURE = 0.1


def npy(t):
    return t.detach().cpu().numpy().astype(np.float32) if torch.is_tensor(t) else t


def perturb_(module: torch.nn.Module, g: torch.Generator) -> None:
    """As make_golden.py: make every parameter non-trivial so that the fixture exercises every term."""
    with torch.no_grad():
        for n, p in module.named_parameters():
            if n.endswith("mlp.2.weight") and "scale_embed" in n:
                p.copy_(0.3 * torch.randn(p.shape, generator=g))
            elif p.ndim == 1:
                p.add_(0.05 * torch.randn(p.shape, generator=g))


def adversarial(g: torch.Generator):
    B, D = 8, 16
    z1 = torch.randn(B, D, generator=g)
    z2 = torch.randn(B, D, generator=g)
    z2[0] = z1[0]                 # a duplicated pair: the positive logit is +1/tau
    z1[1] *= 1e-20                # below eps: the clamp of F.normalize acts, dz = dzh / eps
    z1[2] *= 1e4                  # a long row
    z1[4] = 3.0 * z1[3]           # parallel rows: a negative at +1/tau
    z2[5] = -2.0 * z1[5]          # an anti-parallel positive: the logit is -1/tau
    z2[6] = 0.0                   # an all-zero row
    return z1, z2


def simclr_loss():
    g = torch.Generator().manual_seed(61)
    L = P.SimCLRLoss(temperature=TEMPERATURE)
    cases = {"b3": (torch.randn(3, 5, generator=g), torch.randn(3, 5, generator=g)),
             "b33": (2.0 * torch.randn(33, 130, generator=g), 2.0 * torch.randn(33, 130, generator=g)),
             "b130": (torch.randn(130, 257, generator=g), torch.randn(130, 257, generator=g)),
             "adv": adversarial(g)}
    out = {"temperature": np.float64(TEMPERATURE), "cases": np.array(list(cases))}
    for tag, (z1, z2) in cases.items():
        z1, z2 = z1.clone().requires_grad_(True), z2.clone().requires_grad_(True)
        l = L(z1, z2)
        l.backward()
        out.update({f"{tag}_z1": npy(z1), f"{tag}_z2": npy(z2), f"{tag}_loss": np.float64(l.item()), f"{tag}_dz1": npy(z1.grad),
                    f"{tag}_dz2": npy(z2.grad)})
        print(f"{tag}: loss {l.item():.6f}, max |dz| {max(z1.grad.abs().max().item(), z2.grad.abs().max().item()):.3e}")
    path = os.path.join(HERE, "simclr_loss.npz")
    np.savez_compressed(path, **out)
    print(f"simclr_loss.npz: {os.path.getsize(path) / 1024:.1f} KiB")


def simclr_step_tiny(seed: int = 71):
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(0)
    cfg = dict(img_size=28, patch=14, dim=32, depth=2, heads=2, mlp_ratio=4.0, num_registers=2, scale_aware=True)
    out_dim, B = 64, 4
    student = A.DinoStudentTeacher(A.PatchViT(**cfg), out_dim=out_dim)
    perturb_(student, g)
    with torch.no_grad():
        for v in student.state_dict().values():               # fp16-representable start (stored as float16, exactly)
            v.copy_(v.half().float())
    hp = dict(lr=1e-3, min_lr=1e-5, warmup=2, max_steps=10, wd=0.04, temp=TEMPERATURE)
    opt = torch.optim.AdamW(student.parameters(), lr=hp["lr"], weight_decay=hp["wd"])
    L = P.SimCLRLoss(temperature=TEMPERATURE)
    out = dict(cfg=np.array([28, 14, 32, 2, 2, 2, 1, out_dim], dtype=np.int64),
               hp=np.array([hp[k] for k in ("lr", "min_lr", "warmup", "max_steps", "wd", "temp")], dtype=np.float64))
    out.update({f"init/{k}": v.detach().numpy().astype(np.float16) for k, v in student.state_dict().items()})
    assert all((out[f"init/{k}"].astype(np.float32) == v.detach().numpy()).all() for k, v in student.state_dict().items())
    losses, gns, lrs = [], [], []
    small = {n: torch.zeros_like(p, dtype=torch.bool) for n, p in student.named_parameters()}
    for step in range(3):
        lr = P.get_lr(step, hp["max_steps"], hp["warmup"], hp["lr"], hp["min_lr"])                   # :1692-1700
        for pg in opt.param_groups:
            pg["lr"] = lr
        v1 = torch.randn(B, 3, 28, 28, generator=g)
        v2 = torch.randn(B, 3, 28, 28, generator=g)
        sp = torch.rand(B, 3, generator=g) * 2 + 0.4
        batch, sp2 = torch.cat([v1, v2], 0).half().float(), torch.cat([sp, sp], 0)
        out[f"batch{step}"], out[f"spacing{step}"] = batch.numpy().astype(np.float16), sp2
        feats = student.backbone(batch, spacing=sp2)                                                  # :1729-1737
        s_out = student.head(feats[:, 0])
        loss = L(s_out[:B], s_out[B:])
        loss.backward()                                                                               # :1769-1772, accumulation 1
        tot = 0.0
        for n, p in student.named_parameters():                                                       # :1784-1789
            assert p.grad is not None, n
            tot += p.grad.detach().norm(2).item() ** 2
            out[f"grad{step}/{n}"] = p.grad.detach().clone()
            small[n] |= p.grad.detach().abs() < 1e-6
        opt.step()                                                                                    # :1794-1796; no EMA (:1799)
        opt.zero_grad(set_to_none=True)
        losses.append(loss.item()); gns.append(tot ** 0.5); lrs.append(lr)
    share = sum(int(m.sum()) for m in small.values()) / sum(m.numel() for m in small.values())
    assert share <= 0.10, f"{share:.3f} of the student elements have |g| < 1e-6 in some step: pick another seed"
    out.update({f"student3/{k}": v.detach().clone() for k, v in student.state_dict().items()})
    out["losses"], out["grad_norms"], out["lrs"] = (np.array(v, dtype=np.float64) for v in (losses, gns, lrs))
    out["small_grad_share"] = np.float64(share)
    out["param_order"] = np.array([n for n, _ in student.named_parameters()])
    path = os.path.join(HERE, "simclr_step_tiny.npz")
    np.savez_compressed(path, **{k: (npy(v) if torch.is_tensor(v) else v) for k, v in out.items()})
    print(f"simclr_step_tiny.npz: {os.path.getsize(path) / 1024:.1f} KiB; losses={losses} gn={gns} small-gradient share={share:.4f}")


if __name__ == "__main__":
    only = set(sys.argv[1:])
    for fn in (simclr_loss, simclr_step_tiny):
        if not only or fn.__name__ in only:
            fn()
