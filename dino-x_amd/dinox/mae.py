"""Masked-autoencoder pretraining (``--loss-type mae``) on the HIP kernels.

``MaeDecoder`` / ``MaeModel`` carry the reference's names, constructor arguments, sub-module names and ``state_dict`` keys
(scripts/phase5_big_run.py:816-1023), so its checkpoints load; the tensor work is the masked-token kernels of csrc/mae.hip
(``dinox.ops.mae_*``) around the existing GEMM / LayerNorm / attention nodes:

    noise -> ids_restore, ids_keep                       one launch  (the reference: argsort x 2 + gather)
    patch-embed product on the KEPT patches only         M = V*Lk rows instead of V*L
    [cls | kept patches] + pos                           one launch
    encoder blocks + norm, decoder_embed
    un-shuffle + mask_token + decoder_pos_embed          one launch  (repeat, cat x 2, gather, add)
    decoder blocks + decoder_norm + decoder_pred
    mean over removed patches of the per-patch MSE       two launches, pixels read straight from the image (no patchify copy)

Registers and ``scale_embed`` of the encoder are never used, as in the reference; ``decoder_pos_embed`` is a fixed sin-cos table
(``requires_grad=False``).  There is no CPU path.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict, Optional

import numpy as np
import torch
import torch.nn as nn

from zoo.arch import LayerNorm, Linear, PatchViT, TransformerBlock

from . import ops

__all__ = ["MaeDecoder", "MaeModel", "export_encoder", "sincos_table", "parse_decoder_spec"]


def sincos_table(dim: int, grid: int) -> torch.Tensor:
    """The fixed 2-D sin-cos position table [1, 1 + grid^2, dim] with a zero CLS row, computed in the reference's arithmetic (fp32
    frequencies 1 / 10000^(i / (dim/4)), fp32 products and sin / cos; the first half of the features encodes the column of a patch, the
    second half its row; each half is [sin | cos])."""
    if dim % 4:
        raise ValueError(f"the sin-cos table needs a width that is a multiple of 4, got {dim}")
    quarter = dim // 4
    omega = np.arange(quarter, dtype=np.float32)
    omega /= dim / 4.0
    omega = 1.0 / 10000 ** omega
    cols, rows = np.meshgrid(np.arange(grid, dtype=np.float32), np.arange(grid, dtype=np.float32))

    def half(coord):
        ang = np.outer(coord.reshape(-1), omega)
        return np.concatenate([np.sin(ang), np.cos(ang)], axis=1)

    table = np.concatenate([half(cols), half(rows)], axis=1)
    table = np.concatenate([np.zeros([1, dim]), table], axis=0)
    return torch.from_numpy(table).float().unsqueeze(0)


def parse_decoder_spec(spec: str):
    """'DIMxDEPTHxHEADS' (the reference's decoder is '512x8x16') -> (dim, depth, heads); ValueError with one clear line otherwise."""
    parts = str(spec).lower().split("x")
    try:
        dim, depth, heads = (int(p) for p in parts)
    except ValueError:
        raise ValueError(f"--mae-decoder takes DIMxDEPTHxHEADS (e.g. 512x8x16), got {spec!r}") from None
    if dim < 4 or depth < 1 or heads < 1 or dim % heads or dim % 4:
        raise ValueError(f"--mae-decoder {spec!r}: DIM must be a multiple of 4 and of HEADS, DEPTH and HEADS at least 1")
    return dim, depth, heads


def _run_blocks(blocks, norm, t: torch.Tensor, checkpoint: bool = False) -> torch.Tensor:
    """Blocks + final LayerNorm as PatchViT runs them: where every block is the stock fused node, each LayerNorm but the first rides
    with the product that wrote its input (forward_chained); otherwise block by block.  fp32 output."""
    chain = (not checkpoint and type(norm) is LayerNorm and len(blocks) > 0
             and all(type(b) is TransformerBlock and b._fusable() for b in blocks) and all(b.norm1.eps == norm.eps for b in blocks))
    if chain:
        pre = None
        for i, blk in enumerate(blocks):
            last = i + 1 == len(blocks)
            t, pre = blk.forward_chained(t, pre, norm if last else blocks[i + 1].norm1, torch.float32 if last else None)
        return ops.LayerNormPrecomputedFn.apply(t, norm.weight, norm.bias, *pre)
    for blk in blocks:
        if checkpoint:
            t = torch.utils.checkpoint.checkpoint(blk, t, use_reentrant=False, context_fn=ops.checkpoint_contexts)
        else:
            t = blk(t)
    return norm(t, out_dtype=torch.float32)


class MaeDecoder(nn.Module):
    """Lightweight reconstruction decoder (reference :816-879)."""

    def __init__(self, embed_dim: int, patch_size: int, num_patches: int, decoder_dim: int = 512, decoder_depth: int = 8,
                 decoder_heads: int = 16, mlp_ratio: float = 4.0) -> None:
        super().__init__()
        self.embed_dim = embed_dim
        self.decoder_dim = decoder_dim
        self.num_patches = num_patches
        self.patch_size = patch_size
        self.decoder_embed = Linear(embed_dim, decoder_dim, bias=True)
        self.mask_token = nn.Parameter(torch.zeros(1, 1, decoder_dim))
        self.decoder_pos_embed = nn.Parameter(torch.zeros(1, num_patches + 1, decoder_dim), requires_grad=False)
        self.blocks = nn.ModuleList([TransformerBlock(decoder_dim, decoder_heads, mlp_ratio) for _ in range(decoder_depth)])
        self.decoder_norm = LayerNorm(decoder_dim)
        self.decoder_pred = Linear(decoder_dim, patch_size ** 2 * 3, bias=True)
        self.apply(self._init_weights)

    def _init_weights(self, m: nn.Module) -> None:
        if isinstance(m, nn.Linear):
            nn.init.xavier_uniform_(m.weight)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)
        nn.init.normal_(self.mask_token, std=0.02)      # (re-drawn per visited sub-module, as the reference does: same seed, same weights)

    def forward_full(self, x: torch.Tensor, ids_restore: torch.Tensor, ids_keep: Optional[torch.Tensor] = None) -> torch.Tensor:
        """x [V, 1+Lk, embed_dim] -> [V, 1+L, 3 p^2] in the compute dtype, the CLS row still in front."""
        ops._need_cuda(x, self.mask_token)
        Lk = x.shape[1] - 1
        ids_restore = ids_restore.to(torch.int32)
        if ids_keep is None:      # the ranks of a permutation are the permutation itself: the same kernel returns the kept patches
            ids_restore, ids_keep = ops.mae_mask_ids(ids_restore.float(), Lk)
        e = self.decoder_embed(x)
        xd = ops.MaeUnshuffleFn.apply(e, self.mask_token, self.decoder_pos_embed, ids_restore, ids_keep)
        xd = _run_blocks(self.blocks, self.decoder_norm, xd)
        return self.decoder_pred(xd)

    def forward(self, x: torch.Tensor, ids_restore: torch.Tensor, ids_keep: Optional[torch.Tensor] = None) -> torch.Tensor:
        return self.forward_full(x, ids_restore, ids_keep)[:, 1:, :]


class MaeModel(nn.Module):
    """Encoder + random masking + decoder (reference :882-1023).  ``decoder_depth`` / ``decoder_heads`` extend the reference's
    constructor, which hard-codes 8 and 16."""

    def __init__(self, encoder: PatchViT, decoder_dim: int = 512, mask_ratio: float = 0.75, decoder_depth: int = 8,
                 decoder_heads: int = 16) -> None:
        super().__init__()
        self.encoder = encoder
        self.mask_ratio = mask_ratio
        num_patches = (encoder.img_size // encoder.patch) ** 2
        self.decoder = MaeDecoder(embed_dim=encoder.dim, patch_size=encoder.patch, num_patches=num_patches, decoder_dim=decoder_dim,
                                  decoder_depth=decoder_depth, decoder_heads=decoder_heads)
        self.decoder.decoder_pos_embed.data.copy_(sincos_table(decoder_dim, int(num_patches ** 0.5)))

    @property
    def num_patches(self) -> int:
        return self.decoder.num_patches

    @property
    def len_keep(self) -> int:
        return ops.mae_len_keep(self.num_patches, self.mask_ratio)

    def mask_ids(self, imgs, noise: Optional[torch.Tensor] = None):
        """-> (ids_restore [V, L], ids_keep [V, Lk]) int32.  ``noise=None`` draws ``torch.rand(V, L)`` from torch's global device
        generator, as the reference's random_masking does."""
        V, L = imgs.shape[0], self.num_patches
        if tuple(imgs.shape[1:]) != (3, self.encoder.img_size, self.encoder.img_size):
            raise ValueError(f"mae: images must be [V, 3, {self.encoder.img_size}, {self.encoder.img_size}], got {tuple(imgs.shape)}")
        if not 1 <= self.len_keep < L:
            raise ValueError(f"mae: mask_ratio {self.mask_ratio} keeps {self.len_keep} of {L} patches; at least one must stay and one go")
        if noise is None:
            noise = torch.rand(V, L, device=imgs.device)
        elif tuple(noise.shape) != (V, L):
            raise ValueError(f"mae: noise must be [{V}, {L}], got {tuple(noise.shape)}")
        return ops.mae_mask_ids(noise.to(imgs.device), self.len_keep)

    def forward_full(self, imgs: torch.Tensor, noise: Optional[torch.Tensor] = None):
        """-> (pred_full [V, 1+L, 3 p^2] with the CLS row in front, ids_restore)."""
        if isinstance(imgs, ops.PatchOperand):
            raise ValueError("loss_type='mae' takes the fp32 image batch (the loss reads its pixels), not a PatchOperand")
        enc = self.encoder
        ops._need_cuda(imgs, enc.pos_embed)
        ids_restore, ids_keep = self.mask_ids(imgs, noise)
        t = ops.MaeTokensFn.apply(imgs, enc.patch_embed.weight, enc.patch_embed.bias, enc.cls_token, enc.pos_embed, ids_restore, ids_keep,
                                  enc.patch)
        t = _run_blocks(enc.blocks, enc.norm, t, checkpoint=enc.use_grad_checkpoint and self.training)
        return self.decoder.forward_full(t, ids_restore, ids_keep), ids_restore

    def forward(self, imgs: torch.Tensor, noise: Optional[torch.Tensor] = None):
        """-> (pred [V, L, 3 p^2], mask [V, L] fp32: 0 = kept, 1 = removed)."""
        pred_full, ids_restore = self.forward_full(imgs, noise)
        mask = (ids_restore >= self.len_keep).float()
        return pred_full[:, 1:, :], mask

    def patchify(self, imgs: torch.Tensor) -> torch.Tensor:
        """[V,3,H,W] -> [V, L, 3 p^2], column (py p + px) 3 + c: a host-side view of what the loss kernels index (tests, inspection)."""
        p = self.encoder.patch
        V, _, H, W = imgs.shape
        return imgs.reshape(V, 3, H // p, p, W // p, p).permute(0, 2, 4, 3, 5, 1).reshape(V, (H // p) * (W // p), 3 * p * p)

    def forward_loss(self, imgs: torch.Tensor, pred: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
        """Mean over the removed patches of the per-patch mean squared error (reference :955-969).  ``mask`` is one that this model's
        ``forward`` returned, or any 0 / 1 mask that removes ``L - len_keep`` patches of every sample: the mean divides by
        ``V (L - len_keep)`` and the mask is not read back to the host to count them."""
        if tuple(mask.shape) != (imgs.shape[0], self.num_patches):
            raise ValueError(f"mae: mask must be [{imgs.shape[0]}, {self.num_patches}], got {tuple(mask.shape)}")
        ids = (mask > 0).to(torch.int32) * self.num_patches      # a rank below len_keep where kept, one past every rank where removed
        return ops.MaeLossFn.apply(pred, imgs, ids, self.len_keep, self.encoder.patch, 0)

    def loss(self, imgs: torch.Tensor, noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        """forward + forward_loss without dropping the CLS row of the prediction (no strided copy)."""
        pred_full, ids_restore = self.forward_full(imgs, noise)
        return ops.MaeLossFn.apply(pred_full, imgs, ids_restore, self.len_keep, self.encoder.patch, 1)


def export_encoder(state_dict: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The ``encoder.*`` entries of a MaeModel state dict without the prefix: what ``PatchViT.load_state_dict`` takes."""
    out = OrderedDict((k[len("encoder."):], v) for k, v in state_dict.items() if k.startswith("encoder."))
    if not out:
        raise ValueError("no 'encoder.*' keys: not a MaeModel state dict")
    return out
