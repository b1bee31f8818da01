#!/usr/bin/env python3
"""The MAE step at the headline shape (ViT-S/16, 224 px, batch 256 = 512 views, bf16, decoder 512x8x16, mask ratio 0.75):
  (a) ms/step and samples/s of TrainEngine(loss_type="mae"), next to the dino step of the same encoder and to
  (c) the same MAE step composed from stock PyTorch ops under bf16 autocast (argsort x 2, gather, repeat, cat, patchify, AdamW), written
      here from the description of the objective, on the same device and the same batch;
  (b) the phase split of the mae step between the marks TrainEngine.step records on its launch stream;
  (d) each masked-token kernel alone against its byte count: bytes it must move / a streaming bandwidth.  The bandwidth is
      --hbm-gbs G (the chip figure tools/dma_probe prints) or, without it, a device-to-device copy measured here.
Every timed window ends in a device synchronise; windows alternate between the variants; median [min .. max] over the windows.
--quick: fewer windows and a smaller batch (a profiler's run)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dino-x_amd")]
import numpy as np, torch
import torch.nn as nn
import torch.nn.functional as F
import zoo.arch as arch
from dinox import ops
from dinox.engine import StepHyperParams, TrainEngine
from dinox.mae import MaeModel

QUICK = "--quick" in sys.argv
HBM = float(sys.argv[sys.argv.index("--hbm-gbs") + 1]) if "--hbm-gbs" in sys.argv else None
B, WINDOWS, REPS = (32, 3, 3) if QUICK else (256, 7, 3)            # 7 windows x 3 steps = 21 timed steps per variant
IMG, P, D, DEPTH, HEADS, DD, DDEPTH, DHEADS, RATIO, OUT = 224, 16, 384, 12, 6, 512, 8, 16, 0.75, 8192
DEV = "cuda"
V, L = 2 * B, (IMG // P) ** 2
LK = ops.mae_len_keep(L, RATIO)


def window(fn, reps):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(reps): fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def spread(ts, unit=1e3, name="ms"):
    return f"{np.median(ts)*unit:.3f} {name} [{min(ts)*unit:.3f} .. {max(ts)*unit:.3f}]"


g = torch.Generator().manual_seed(0)
batch = torch.randn(V, 3, IMG, IMG, generator=g).to(DEV)
sp = (torch.rand(B, 3, generator=g) * 2 + 0.4).repeat(2, 1).to(DEV)
kw = dict(img_size=IMG, patch=P, dim=D, depth=DEPTH, heads=HEADS, num_registers=4, scale_aware=True)
hp = dict(lr=1e-4, warmup_steps=10)


# ---- (c) the MAE step in stock PyTorch ops
class PlainBlock(nn.Module):
    def __init__(self, dim, heads):
        super().__init__()
        self.heads = heads
        self.n1, self.n2 = nn.LayerNorm(dim), nn.LayerNorm(dim)
        self.qkv, self.proj = nn.Linear(dim, 3 * dim), nn.Linear(dim, dim)
        self.fc1, self.fc2 = nn.Linear(dim, 4 * dim), nn.Linear(4 * dim, dim)

    def forward(self, x):
        b, n, d = x.shape
        q, k, v = self.qkv(self.n1(x)).view(b, n, 3, self.heads, d // self.heads).permute(2, 0, 3, 1, 4)
        x = x + self.proj(F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(b, n, d))
        return x + self.fc2(F.gelu(self.fc1(self.n2(x))))


class PlainMae(nn.Module):
    def __init__(self):
        super().__init__()
        self.embed = nn.Conv2d(3, D, P, P)
        self.cls, self.pos = nn.Parameter(torch.zeros(1, 1, D)), nn.Parameter(torch.randn(1, 1 + L, D) * 0.02)
        self.enc, self.enc_norm = nn.ModuleList(PlainBlock(D, HEADS) for _ in range(DEPTH)), nn.LayerNorm(D)
        self.to_dec = nn.Linear(D, DD)
        self.mask_token = nn.Parameter(torch.randn(1, 1, DD) * 0.02)
        self.register_buffer("dec_pos", torch.randn(1, 1 + L, DD) * 0.02)
        self.dec, self.dec_norm = nn.ModuleList(PlainBlock(DD, DHEADS) for _ in range(DDEPTH)), nn.LayerNorm(DD)
        self.to_pix = nn.Linear(DD, 3 * P * P)

    def forward(self, x):
        v = x.shape[0]
        t = self.embed(x).flatten(2).transpose(1, 2) + self.pos[:, 1:]
        shuffle = torch.argsort(torch.rand(v, L, device=x.device), dim=1)
        restore = torch.argsort(shuffle, dim=1)
        t = torch.gather(t, 1, shuffle[:, :LK, None].expand(-1, -1, D))
        t = torch.cat([(self.cls + self.pos[:, :1]).expand(v, -1, -1), t], 1)
        for blk in self.enc:
            t = blk(t)
        t = self.to_dec(self.enc_norm(t))
        body = torch.cat([t[:, 1:], self.mask_token.expand(v, L - LK, -1).to(t.dtype)], 1)
        body = torch.gather(body, 1, restore[:, :, None].expand(-1, -1, DD))
        t = torch.cat([t[:, :1], body], 1) + self.dec_pos
        for blk in self.dec:
            t = blk(t)
        pred = self.to_pix(self.dec_norm(t))[:, 1:]
        target = x.view(v, 3, IMG // P, P, IMG // P, P).permute(0, 2, 4, 3, 5, 1).reshape(v, L, 3 * P * P)
        per_patch = ((pred.float() - target) ** 2).mean(-1)
        removed = (restore >= LK).float()
        return (per_patch * removed).sum() / removed.sum()


torch.manual_seed(1)
plain = PlainMae().to(DEV)
plain_opt = torch.optim.AdamW(plain.parameters(), lr=1e-4, weight_decay=0.04)


def plain_step():
    plain_opt.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss = plain(batch)
    loss.backward()
    plain_opt.step()
    return loss


# ---- (a) the engines
torch.manual_seed(1)
mae_model = MaeModel(arch.PatchViT(**kw), decoder_dim=DD, mask_ratio=RATIO, decoder_depth=DDEPTH, decoder_heads=DHEADS).to(DEV)
mae_eng = TrainEngine(mae_model, None, OUT, StepHyperParams(loss_type="mae", mae_mask_ratio=RATIO, **hp), amp_dtype=torch.bfloat16)
torch.manual_seed(1)
s_ = arch.DinoStudentTeacher(arch.PatchViT(**kw), OUT)
t_ = arch.DinoStudentTeacher(arch.PatchViT(**kw), OUT)
t_.load_state_dict(s_.state_dict())
dino_eng = TrainEngine(s_.to(DEV), t_.to(DEV), OUT, StepHyperParams(loss_type="dino", **hp), amp_dtype=torch.bfloat16)
variants = {"mae step (HIP engine)": lambda: mae_eng.step(batch, None), "dino step (HIP engine)": lambda: dino_eng.step(batch, sp),
            "mae step (stock PyTorch ops, bf16 autocast)": plain_step}
for fn in variants.values():
    for _ in range(3): fn()
times = {k: [] for k in variants}
for _ in range(WINDOWS):
    for k, fn in variants.items():
        times[k].append(window(fn, REPS))
for k, ts in times.items():
    print(f"(a) {k}, ViT-S/16 {IMG} bs {B} ({V} views) bf16, decoder {DD}x{DDEPTH}x{DHEADS}: {spread(ts)} = {B/np.median(ts):.0f} samples/s")
print(f"    losses: mae {mae_eng.scalars()['loss']:.4f}, dino {dino_eng.scalars()['loss']:.4f}, stock mae {float(plain_step().detach()):.4f}")

# ---- (b) phase split of the mae step
acc, n = {}, 4
for _ in range(n):
    mae_eng.marks = []
    mae_eng.step(batch, None)
    torch.cuda.synchronize()
    m = mae_eng.marks
    for (_, e0), (name, e1) in zip(m[:-1], m[1:]):
        acc[name] = acc.get(name, 0.0) + e0.elapsed_time(e1)
mae_eng.marks = None
print("(b) mae step, ms between the marks: " + ", ".join(f"{k} {v / n:.3f}" for k, v in acc.items()))
del mae_eng, dino_eng, plain, plain_opt, variants
torch.cuda.empty_cache()

# ---- (d) each masked-token kernel against its byte count
if HBM is None:
    a_, b_ = torch.empty(1 << 28, dtype=torch.float32, device=DEV), torch.empty(1 << 28, dtype=torch.float32, device=DEV)
    for _ in range(3): b_.copy_(a_)
    HBM = 2 * a_.numel() * 4 / min(window(lambda: b_.copy_(a_), 10) for _ in range(5)) / 1e9
    del a_, b_
    print(f"(d) streaming bandwidth: {HBM:.0f} GB/s (a 1 GiB device-to-device copy, read + write, measured here)")
else:
    print(f"(d) streaming bandwidth: {HBM:.0f} GB/s (given)")
bf = torch.bfloat16
K = 3 * P * P
lib, p = ops.lib, lambda t: t.data_ptr()
st = torch.cuda.current_stream().cuda_stream
noise = torch.rand(V, L, device=DEV)
ids_restore, ids_keep = ops.mae_mask_ids(noise, LK)
f32 = lambda *sh: torch.empty(sh, dtype=torch.float32, device=DEV)
patches, dpatches = torch.randn(V * LK, D, device=DEV).to(bf), torch.empty(V * LK, D, dtype=bf, device=DEV)
cls, pos, tok = torch.randn(1, 1, D, device=DEV), torch.randn(1, 1 + L, D, device=DEV), f32(V, 1 + LK, D)
dcls, dpos = f32(D), f32(1 + L, D)
e, de = torch.randn(V, 1 + LK, DD, device=DEV).to(bf), torch.empty(V, 1 + LK, DD, dtype=bf, device=DEV)
mtok, dec_pos, xd = torch.randn(1, 1, DD, device=DEV), torch.randn(1, 1 + L, DD, device=DEV), torch.randn(V, 1 + L, DD, device=DEV)
dmask, ws = f32(DD), f32(V, DD)
pred = torch.randn(V, 1 + L, K, device=DEV).to(bf)
_, saved = ops.mae_loss_fwd(pred, batch, ids_restore, LK, P, lead=1)
rem = V * (L - LK)
kernels = {      # name: (call, bytes it must move)
    "mae_mask_ids": (lambda: ops.mae_mask_ids(noise, LK), V * L * 8 + V * LK * 4),
    "mae_gather_unfold": (lambda: ops.mae_gather_unfold(batch, ids_keep, P, bf), V * LK * K * 6 + V * LK * 4),
    "mae_tokens_fwd": (lambda: lib.dinox_mae_tokens_fwd(p(patches), p(cls), p(pos), p(ids_keep), p(tok), V, L, LK, D, 1, st),
                       V * LK * D * 2 + V * (1 + LK) * D * 4 + (1 + L) * D * 4),
    "mae_tokens_bwd": (lambda: lib.dinox_mae_tokens_bwd(p(tok), p(ids_restore), p(dpatches), p(dcls), p(dpos), V, L, LK, D, 1, st),
                       V * (1 + LK) * D * 4 + V * LK * D * 2 + (1 + L) * D * 4),
    "mae_unshuffle_fwd": (lambda: lib.dinox_mae_unshuffle_fwd(p(e), p(mtok), p(dec_pos), p(ids_restore), p(xd), V, L, LK, DD, 1, st),
                          V * (1 + LK) * DD * 2 + V * (1 + L) * DD * 4 + (1 + L) * DD * 4 + V * L * 4),
    "mae_unshuffle_bwd": (lambda: lib.dinox_mae_unshuffle_bwd(p(xd), p(ids_keep), p(ids_restore), p(de), p(dmask), p(ws), V, L, LK, DD, 1, st),
                          V * (1 + L) * DD * 4 + V * (1 + LK) * DD * 2 + V * L * 4),
    "mae_loss_fwd": (lambda: ops.mae_loss_fwd(pred, batch, ids_restore, LK, P, lead=1), rem * K * 6 + V * L * 4),
    "mae_loss_bwd": (lambda: ops.mae_loss_bwd(saved, 1.0), rem * K * 6 + V * (1 + L) * K * 2 + V * L * 4),
}
assert ops._code(bf) == 1
for k, (fn, nbytes) in kernels.items():
    for _ in range(3): fn()
    ts = [window(fn, 50) for _ in range(3 if QUICK else 5)]
    floor = nbytes / (HBM * 1e9)
    print(f"    {k}: {spread(ts, 1e6, 'us')}; {nbytes / 1e6:.1f} MB -> {floor * 1e6:.1f} us at the streaming bandwidth, "
          f"{100 * floor / np.median(ts):.0f} % of it reached")
