"""Float64 statements of the iBOT kernels (csrc/ibot.hip), their fp32 error bounds, and a plain-torch statement of the whole training
objective with the masked-patch term.  Style and constants of tests/_small_kernels_oracle.py: a bound has the form (n_ops + 2) u S, the
tolerance of expf / logf is the project's CE_LOSS_RTOL / CE_DS_RTOL.  No new constant."""
import math

import numpy as np
import torch

import _small_kernels_oracle as SO
from _small_kernels_oracle import CE_DS_RTOL, CE_LOSS_RTOL, F64, TINY, U, block_adds, dino_inputs, f32  # noqa: F401  (re-exported to the tests)

MASK_CHUNK = 64      # csrc/ibot.hip IBOT_MASK_CHUNK


# ------------------------------------------------------------------------------------------ cross-entropy
def ibot_ce(s, t, center, w, ts, tt, scale=1.0, grad_scale=1.0, dt=F64):
    """row[m] = -sum_k softmax((t[m] - c) / tt)[k] log_softmax(s[m] / ts)[k];  loss = scale sum_m w[m] row[m];
    ds[m] = grad_scale scale w[m] (softmax(s[m] / ts) - p_t[m]) / ts.  The row parts come from the DINO oracle with every student row
    scored against the teacher row of the same index (no view pairing)."""
    M = np.asarray(s).shape[0]
    o = SO._dino(s, t, center, ts, tt, [[m] for m in range(M)], 1.0, [1] * M, 1.0, dt)
    w = np.asarray(w, dt).reshape(-1)
    gs = dt(f32(grad_scale)) * dt(f32(scale))
    o["w"], o["gs"], o["scale"] = w, float(gs), float(f32(scale))
    o["ds"] = gs * w[:, None] * (o["p"] - o["tpi"]) / dt(f32(ts))
    o["loss"] = dt(f32(scale)) * (w * o["row"]).sum()
    o["ts"] = float(f32(ts))
    return o


def bound_ibot(o):
    """bound_dino without the pairing, plus the weights: g = (grad_scale * scale) * w[m] is two rounded multiplies in front of the
    DINO kernel's four operations on |p| + |tp|; the loss multiplies every row by w[m] (1) before the 256-thread sum, then by scale (1)."""
    b = SO.bound_dino(o)               # (its "ds" and "loss" are for coef = 1, grad_scale = 1: rebuilt below; "row" is what it is)
    K = o["zs"].shape[1]
    ns = block_adds(K)
    da_s = (4 + 2) * U * (np.abs(o["zs"]) + np.abs(o["ms"]))
    da_t = (4 + 2) * U * (np.abs(o["zt"]) + np.abs(o["mt"]))
    rel_ss = (o["es"] * da_s).sum(1, keepdims=True) / o["ss"] + (ns + 2) * U
    rel_st = (o["et"] * da_t).sum(1, keepdims=True) / o["st"] + (ns + 2) * U
    dtp = o["tp"] * (da_t + rel_st + 2 * U)
    dp = o["p"] * (da_s + rel_ss + 2 * U)
    c = np.abs(o["gs"] * o["w"] / o["ts"])[:, None]
    ds = c * (dp + dtp + (4 + 2 + 2) * U * (o["p"] + o["tp"])) + TINY
    aw = np.abs(o["w"])
    n = len(o["row"])
    loss = abs(o["scale"]) * ((aw * b["row"]).sum() + (block_adds(n) + 2 + 2) * U * (aw * np.abs(o["row"])).sum()) + TINY
    return {"row": b["row"], "ds": ds, "loss": loss}


def ibot_ce_torch(s, t, center, w, ts, tt, scale=1.0, grad_scale=1.0):
    """The definition, literally, in torch float64 with autograd: (loss, grad_scale * d loss / d s)."""
    s = torch.tensor(np.asarray(s, F64), requires_grad=True)
    t, c, w = (torch.tensor(np.asarray(x, F64)) for x in (t, center, w))
    ts, tt, scale, grad_scale = float(f32(ts)), float(f32(tt)), float(f32(scale)), float(f32(grad_scale))
    p_t = torch.softmax((t - c.reshape(1, -1)) / tt, dim=-1)
    row = -(p_t * torch.log_softmax(s / ts, dim=-1)).sum(-1)
    loss = scale * (w * row).sum()
    loss.backward()
    return loss.detach().numpy(), grad_scale * s.grad.numpy()


# ------------------------------------------------------------------------------------------ mask token, gather, scatter
def round_to(x, bf16):
    x = np.asarray(x, np.float32)
    return torch.from_numpy(x).bfloat16().float().numpy() if bf16 else x


def put_mask(patches, mask_token, idx, bf16):
    out = np.array(patches, np.float32, copy=True)
    out[np.asarray(idx, np.int64)] = round_to(mask_token, bf16)
    return out


def put_mask_bwd(dpatches, idx):
    """-> (dmask float64, its |.| sum, dpatches with the masked rows zeroed)."""
    idx = np.asarray(idx, np.int64)
    rows = np.asarray(dpatches, F64)[idx]
    out = np.array(dpatches, np.float32, copy=True)
    out[idx] = 0.0
    return rows.sum(0), np.abs(rows).sum(0), out


def example_masks(V, P):
    """Masks with an empty view and a fully masked view (V >= 3), a lone patch, and a scattered one of more than one chunk when it fits."""
    full = np.concatenate([np.arange(1 * P, 2 * P), [2 * P + P // 2]])                 # view 0 empty, view 1 full, one patch of view 2
    lone = np.array([V * P - 1])
    r = np.random.default_rng(5)
    many = np.sort(r.choice(V * P, size=min(V * P - 1, MASK_CHUNK + 7), replace=False))
    return {"empty+full": full.astype(np.int32), "lone": lone.astype(np.int32), "scattered": many.astype(np.int32)}


# ------------------------------------------------------------------------------------------ the whole objective in plain torch
def masked_vit_forward(O, p, x, spacing, cfg, pre, flat_idx):
    """oracle.vit_forward with the embedding of the patches ``flat_idx`` (v * P + i) replaced by mask_token after the patch-embedding
    product, before pos_embed / the scale embedding."""
    B = x.shape[0]
    t = O.patch_embed(x, p[pre + "patch_embed.weight"], p[pre + "patch_embed.bias"], cfg.patch)
    P, D = t.shape[1], t.shape[2]
    hit = torch.zeros(B * P, dtype=torch.bool)
    hit[torch.as_tensor(np.asarray(flat_idx, np.int64))] = True
    t = torch.where(hit.view(B, P, 1), p[pre + "mask_token"].expand(B, P, D), t)
    t = torch.cat([p[pre + "cls_token"].expand(B, -1, -1), t], dim=1)
    t = t + p[pre + "pos_embed"]
    if cfg.scale_aware and spacing is not None:
        t = t + O.scale_embedding(spacing, p, pre + "scale_embed.")
    if cfg.num_registers > 0:
        t = torch.cat([t, p[pre + "registers"].expand(B, -1, -1)], dim=1)
    for i in range(cfg.depth):
        t = O.block(t, p, f"{pre}blocks.{i}.", cfg.heads)
    return O.layer_norm(t, p[pre + "norm.weight"], p[pre + "norm.bias"])


def objective(O, cfg, student, teacher, center, ibot_center, batch, sp2, mask, hp, ibot_weight, locs=None, spl=None, centering="ema",
              sk_iters=3):
    """loss = L_dino + gram_weight L_gram + ibot_weight L_ibot on CPU tensors, with autograd: (scalars, gradient of every student
    parameter).  ``mask``: a dinox.ibot.PatchMask on the host.  ``centering="sinkhorn"``: both centres come from this step's teacher rows."""
    import _sinkhorn_oracle as SK
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in student.items()}
    idx, w, tok = (torch.as_tensor(np.asarray(a)) for a in mask.triple())
    V = batch.shape[0]
    s_feats = masked_vit_forward(O, leaves, batch, sp2, cfg, "backbone.", idx) if len(idx) else O.vit_forward(leaves, batch, sp2, cfg, pre="backbone.")
    with torch.no_grad():
        t_feats = O.vit_forward(teacher, batch, sp2, cfg, pre="backbone.")
        t_out = O.head_forward(teacher, t_feats[:, 0])
        t_p = O.head_forward(teacher, t_feats.reshape(-1, t_feats.shape[-1])[tok.long()])
        if centering == "sinkhorn":
            center = torch.from_numpy(SK.sk_center(t_out.numpy(), hp.teacher_temp, sk_iters)).float().reshape(1, -1)
            if len(idx):
                ibot_center = torch.from_numpy(SK.sk_center(t_p.numpy(), hp.teacher_temp, sk_iters)).float().reshape(1, -1)
    s_out = O.head_forward(leaves, s_feats[:, 0])
    if locs is not None:
        l_feats = O.vit_forward(leaves, locs, spl, cfg, pre="backbone.")
        s_all = torch.cat([s_out, O.head_forward(leaves, l_feats[:, 0])], dim=0)
        l_dino = O.dino_loss_multicrop(s_all, t_out, center, hp.student_temp, hp.teacher_temp)
    else:
        l_dino = O.dino_loss(s_out, t_out, center, hp.student_temp, hp.teacher_temp)
    l_gram = O.gram_loss(s_feats, t_feats)
    if len(idx):
        s_p = O.head_forward(leaves, s_feats.reshape(-1, s_feats.shape[-1])[tok.long()])
        p_t = O.softmax_lastdim((t_p - ibot_center) / hp.teacher_temp)
        row = -(p_t * O.log_softmax_lastdim(s_p / hp.student_temp)).sum(-1)
        l_ibot = (w * row).sum() / V
    else:
        l_ibot = torch.zeros(())
    loss = l_dino + hp.gram_weight * l_gram + ibot_weight * l_ibot
    loss.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}
    norm = math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads.values()))
    sc = {"loss": loss, "dino": l_dino, "gram": l_gram, "ibot": l_ibot}
    return dict({k: float(v.detach()) for k, v in sc.items()}, grad_norm=norm), grads, t_p
