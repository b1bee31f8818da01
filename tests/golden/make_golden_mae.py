#!/usr/bin/env python3
"""Generate the MAE fixtures in this directory FROM THE REAL REFERENCE (same arrangement as make_golden_simclr.py: the reference
checkout is imported by path, runs on the CPU in fp32 with seeded inputs, and only data is written).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_mae.py        (DINOX_REFERENCE: the reference checkout)

Fixtures
  mae_parts.npz            the reference's own random_masking (+ the pos / CLS assembly of MaeModel.forward), the un-shuffle of
                           MaeDecoder.forward (a depth-0 decoder whose three layers are identities) and patchify / forward_loss, each
                           with autograd under a seeded upstream gradient, for (V, L, Lk, D, p) = (2, 16, 4, 8, 4), (3, 196, 49, 40, 4)
                           and (2, 4, 1, 8, 14).  The noise is what torch.rand drew inside random_masking (re-drawn from the same seed
                           and checked against the returned ids_restore); asserted free of ties.
  mae_step_tiny.npz        three steps of the reference loop order in mae mode (:1627-1632, :1692-1700, :1724-1727, :1769-1796) on a
                           32/8/32/2/2 scale-aware encoder with 2 registers and a MaeDecoder(32, depth 2, heads 4), batches of 6 images:
                           initial weights and batches (fp16-representable, stored as float16; the sin-cos table as float32), the noise of
                           every step (torch seeded immediately before each forward), per-step loss / grad-norm / lr / mask, every
                           parameter gradient of steps 0 and 2, the names of the parameters whose grad is None.  grad_norms is what the
                           loop logs: over student.parameters(), i.e. the ENCODER's gradients (:1785); grad_norms_all covers the decoder too.
  mae_step_tiny_more.npz   the model after step 3, per reached parameter the elements whose gradient was below 1e-6 in some step
                           (1 % of them: the key biases, which the softmax cancels), and step 0 once more under torch.autocast("cpu", bfloat16) (loss and gradients): the
                           autocast twin of the bf16 gate.  (A file of its own: together they would pass the 1 MiB limit.)
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

MASK_RATIO = 0.75
CASES = {"s16": (2, 16, 4, 8, 4), "s196": (3, 196, 49, 40, 4), "p14": (2, 4, 1, 8, 14)}


def npy(t):
    return t.detach().cpu().numpy().astype(np.float32) if torch.is_tensor(t) else t


def perturb_(module: torch.nn.Module, g: torch.Generator) -> None:
    """As make_golden.py: make every parameter non-trivial so that the fixture exercises every term."""
    with torch.no_grad():
        for n, p in module.named_parameters():
            if not p.requires_grad:
                continue
            if n.endswith("mlp.2.weight") and "scale_embed" in n:
                p.copy_(0.3 * torch.randn(p.shape, generator=g))
            elif p.ndim == 1:
                p.add_(0.05 * torch.randn(p.shape, generator=g))


def mae_parts():
    g = torch.Generator().manual_seed(83)
    out = {"mask_ratio": np.float64(MASK_RATIO), "cases": np.array(list(CASES))}
    for ci, (tag, (V, L, Lk, D, p)) in enumerate(CASES.items()):
        out[f"{tag}_dims"] = np.array([V, L, Lk, D, p], dtype=np.int64)
        rnd = lambda *s: torch.randn(*s, generator=g)
        # -- encoder side: MaeModel.forward steps 2-4 (:1004-1013) around the reference's random_masking
        patches = rnd(V, L, D).requires_grad_(True)
        pos = rnd(1, 1 + L, D).requires_grad_(True)
        cls = rnd(1, 1, D).requires_grad_(True)
        seed = 500 + ci
        torch.manual_seed(seed)
        x_masked, mask, ids_restore = P.MaeModel.random_masking(None, patches + pos[:, 1:, :], MASK_RATIO)
        torch.manual_seed(seed)
        noise = torch.rand(V, L)
        assert all(len(set(row.tolist())) == L for row in noise), "ties in the noise: pick another seed"
        assert torch.equal(torch.argsort(torch.argsort(noise, dim=1), dim=1), ids_restore) and x_masked.shape[1] == Lk
        tok = torch.cat([(cls + pos[:, :1, :]).expand(V, -1, -1), x_masked], dim=1)
        gtok = rnd(V, 1 + Lk, D)
        tok.backward(gtok)
        out.update({f"{tag}_noise": npy(noise), f"{tag}_ids_restore": ids_restore.numpy().astype(np.int32), f"{tag}_mask": npy(mask),
                    f"{tag}_patches": npy(patches), f"{tag}_pos": npy(pos), f"{tag}_cls": npy(cls), f"{tag}_tok": npy(tok),
                    f"{tag}_gtok": npy(gtok), f"{tag}_dpatches": npy(patches.grad), f"{tag}_dpos": npy(pos.grad), f"{tag}_dcls": npy(cls.grad)})
        # -- decoder side: the un-shuffle of MaeDecoder.forward (:864-870) -- no blocks, identity layers
        dec = P.MaeDecoder(embed_dim=D, patch_size=p, num_patches=L, decoder_dim=D, decoder_depth=0, decoder_heads=1)
        dec.decoder_embed = dec.decoder_norm = dec.decoder_pred = torch.nn.Identity()
        with torch.no_grad():
            dec.mask_token.copy_(rnd(1, 1, D))
            dec.decoder_pos_embed.copy_(rnd(1, 1 + L, D))
        e = rnd(V, 1 + Lk, D).requires_grad_(True)
        xd = dec(e, ids_restore)                                   # [V, L, D]: the CLS row is dropped by the reference
        gxd = rnd(V, L, D)
        xd.backward(gxd)
        assert dec.decoder_pos_embed.grad is None
        out.update({f"{tag}_e": npy(e), f"{tag}_mask_token": npy(dec.mask_token), f"{tag}_dec_pos": npy(dec.decoder_pos_embed),
                    f"{tag}_xd": npy(xd), f"{tag}_gxd": npy(gxd), f"{tag}_de": npy(e.grad), f"{tag}_dmask_token": npy(dec.mask_token.grad)})
        # -- loss: patchify + forward_loss (:941-969)
        side = int(round(L ** 0.5)) * p
        ns = types.SimpleNamespace(encoder=types.SimpleNamespace(patch=p))
        ns.patchify = lambda imgs, ns=ns: P.MaeModel.patchify(ns, imgs)
        imgs = rnd(V, 3, side, side)
        pred = rnd(V, L, 3 * p * p).requires_grad_(True)
        loss = P.MaeModel.forward_loss(ns, imgs, pred, mask)
        gscale = 0.5
        (loss * gscale).backward()
        out.update({f"{tag}_imgs": npy(imgs), f"{tag}_pred": npy(pred), f"{tag}_loss": np.float64(loss.item()), f"{tag}_gscale": np.float64(gscale), f"{tag}_dpred": npy(pred.grad)})
        print(f"{tag}: loss {loss.item():.6f}, removed {int(mask.sum())} of {V * L}")
    path = os.path.join(HERE, "mae_parts.npz")
    np.savez_compressed(path, **out)
    print(f"mae_parts.npz: {os.path.getsize(path) / 1024:.1f} KiB")
    assert os.path.getsize(path) < (1 << 20)


def build_tiny():
    cfg = dict(img_size=32, patch=8, dim=32, depth=2, heads=2, mlp_ratio=4.0, num_registers=2, scale_aware=True)
    enc = A.PatchViT(**cfg)
    mae = P.MaeModel(enc, mask_ratio=MASK_RATIO)
    mae.decoder = P.MaeDecoder(embed_dim=32, patch_size=8, num_patches=16, decoder_dim=32, decoder_depth=2, decoder_heads=4)
    mae.decoder.decoder_pos_embed.data.copy_(mae._get_2d_sincos_pos_embed(32, 4, cls_token=True))
    return enc, mae


def mae_step_tiny(seed: int = 91):
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(0)
    enc, mae = build_tiny()
    perturb_(mae, g)
    with torch.no_grad():
        for n, v in mae.state_dict().items():                 # fp16-representable start (stored as float16, exactly)
            if n != "decoder.decoder_pos_embed":
                v.copy_(v.half().float())
    n_params = sum(p.numel() for p in mae.parameters())
    hp = dict(lr=1e-3, min_lr=1e-5, warmup=2, max_steps=10, wd=0.04)
    B = 6
    opt = torch.optim.AdamW(mae.parameters(), lr=hp["lr"], weight_decay=hp["wd"])                      # :1632
    out = dict(cfg=np.array([32, 8, 32, 2, 2, 2, 1, 32, 2, 4], dtype=np.int64),       # img patch dim depth heads registers scale_aware | decoder dim depth heads
               hp=np.array([hp[k] for k in ("lr", "min_lr", "warmup", "max_steps", "wd")] + [MASK_RATIO], dtype=np.float64),
               n_params=np.int64(n_params))
    init = {k: v.detach().clone() for k, v in mae.state_dict().items()}
    for k, v in init.items():
        out[f"init/{k}"] = v.numpy().astype(np.float32 if k == "decoder.decoder_pos_embed" else np.float16)
        assert (out[f"init/{k}"].astype(np.float32) == v.numpy()).all(), k
    more = {}
    # the autocast twin of step 0 (before the fp32 run touches the weights)
    batches = [torch.randn(B, 3, 32, 32, generator=g).half().float() for _ in range(3)]
    torch.manual_seed(1000)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        pred, mask = mae(batches[0])
        loss_ac = mae.forward_loss(batches[0], pred, mask)
    loss_ac.backward()
    more["autocast_loss0"] = np.float64(loss_ac.item())
    for n, p in mae.named_parameters():
        if p.grad is not None:
            more[f"autocast_grad0/{n}"] = p.grad.detach().clone().float()
    opt.zero_grad(set_to_none=True)

    losses, gns, gns_all, lrs, none_names = [], [], [], [], None
    small = {n: torch.zeros_like(p, dtype=torch.bool) for n, p in mae.named_parameters()}
    for step in range(3):
        lr = P.get_lr(step, hp["max_steps"], hp["warmup"], hp["lr"], hp["min_lr"])                   # :1692-1700
        for pg in opt.param_groups:
            pg["lr"] = lr
        batch = batches[step]
        out[f"batch{step}"] = batch.numpy().astype(np.float16)
        torch.manual_seed(1000 + step)
        noise = torch.rand(B, 16)
        torch.manual_seed(1000 + step)
        pred, mask = mae(batch)                                                                       # :1725
        loss = mae.forward_loss(batch, pred, mask)                                                    # :1726
        assert all(len(set(r.tolist())) == 16 for r in noise)
        assert torch.equal((torch.argsort(torch.argsort(noise, dim=1), dim=1) >= 4).float(), mask)
        out[f"noise{step}"], out[f"mask{step}"] = noise.clone(), mask.clone()
        loss.backward()                                                                               # :1769-1772, accumulation 1
        tot = sum(p.grad.detach().norm(2).item() ** 2 for p in enc.parameters() if p.grad is not None)   # :1784-1789 (student = the encoder + an unused head)
        tot_all = sum(p.grad.detach().norm(2).item() ** 2 for p in mae.parameters() if p.grad is not None)
        nn_ = [n for n, p in mae.named_parameters() if p.grad is None]
        assert none_names is None or none_names == nn_
        none_names = nn_
        for n, p in mae.named_parameters():
            if p.grad is not None:
                if step != 1:
                    out[f"grad{step}/{n}"] = p.grad.detach().clone()
                small[n] |= p.grad.detach().abs() < 1e-6
        opt.step()                                                                                    # :1794-1796; no EMA (:1799)
        opt.zero_grad(set_to_none=True)
        losses.append(loss.item()); gns.append(tot ** 0.5); gns_all.append(tot_all ** 0.5); lrs.append(lr)
    reached = [n for n in small if n not in none_names]
    share = sum(int(small[n].sum()) for n in reached) / sum(small[n].numel() for n in reached)
    assert share <= 0.10, f"{share:.3f} of the reached elements have |g| < 1e-6 in some step: pick another seed"
    for n in none_names:                                                                              # untouched by AdamW, to the bit
        assert torch.equal(dict(mae.named_parameters())[n].detach(), init[n]), n
    more.update({f"student3/{k}": v.detach().clone() for k, v in mae.state_dict().items()})
    more.update({f"small/{n}": small[n].numpy() for n in reached})       # |g| < 1e-6 in some step: Adam moves such an element by +-lr of round-off sign
    out["losses"], out["grad_norms"], out["grad_norms_all"], out["lrs"] = (np.array(v, dtype=np.float64) for v in (losses, gns, gns_all, lrs))
    out["small_grad_share"] = np.float64(share)
    out["param_order"] = np.array([n for n, _ in mae.named_parameters()])
    out["param_shapes"] = np.array(["x".join(str(d) for d in p.shape) for _, p in mae.named_parameters()])
    out["grad_none"] = np.array(none_names)
    for fname, d in (("mae_step_tiny.npz", out), ("mae_step_tiny_more.npz", more)):
        path = os.path.join(HERE, fname)
        np.savez_compressed(path, **{k: (npy(v) if torch.is_tensor(v) else v) for k, v in d.items()})
        print(f"{fname}: {os.path.getsize(path) / 1024:.1f} KiB")
        assert os.path.getsize(path) < (1 << 20)
    print(f"params={n_params} losses={losses} gn={gns} gn_all={gns_all} autocast loss0={loss_ac.item()} small-gradient share={share:.4f} "
          f"grad None: {none_names}")


if __name__ == "__main__":
    only = set(sys.argv[1:])
    for fn in (mae_parts, mae_step_tiny):
        if not only or fn.__name__ in only:
            fn()
