#!/usr/bin/env python3
"""Generate monitor_tiny.npz FROM THE REAL REFERENCE (same arrangement as make_golden.py: the reference checkout is imported by
path, runs on the CPU in fp32 with seeded inputs, and only data is written).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_monitor.py        (DINOX_REFERENCE: the reference checkout)

monitor_tiny.npz   a 56 px / patch 14 / dim 64 / depth 2 / heads 2 / 2 registers backbone (seed 0, 1-D parameters perturbed so that
                   LayerNorms and biases are not trivial) on 8 seeded images:
                     state.<key>          the DinoStudentTeacher state dict (out_dim 32)
                     batch                [8, 3, 56, 56]
                     feats                the reference backbone's output [8, 1 + 16 + 2, 64]
                     heatmap              make_attention_heatmap(model, batch[i:i+1]) (phase5_big_run.py:85-113) for every image i: [8, 4, 4]
                     embedding_std_mean,  the two statistics of phase5_monitor.py:245-247 on the 8 CLS embeddings
                     embedding_norm_mean
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

CFG = dict(img_size=56, patch=14, dim=64, depth=2, heads=2, num_registers=2)


def main() -> None:
    torch.manual_seed(0)
    model = A.DinoStudentTeacher(A.PatchViT(**CFG), out_dim=32)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for _, p in model.named_parameters():
            if p.ndim == 1:
                p.add_(0.05 * torch.randn(p.shape, generator=g))
    batch = torch.randn(8, 3, 56, 56, generator=g)
    heat = np.stack([P.make_attention_heatmap(model, batch[i:i + 1]) for i in range(8)], 0).astype(np.float32)
    model.eval()
    with torch.no_grad():
        feats = model.backbone(batch)
    E = feats[:, 0, :]
    std = E.std(dim=0).mean().item()            # phase5_monitor.py:245-247
    norm = E.norm(dim=-1).mean().item()
    out = {"state." + k: v.detach().numpy().astype(np.float32) for k, v in model.state_dict().items()}
    out.update(batch=batch.numpy(), feats=feats.numpy().astype(np.float32), heatmap=heat,
               embedding_std_mean=np.float64(std), embedding_norm_mean=np.float64(norm))
    path = os.path.join(HERE, "monitor_tiny.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes, heatmap {heat.shape}, std {std:.6f}, norm {norm:.6f}")


if __name__ == "__main__":
    main()
