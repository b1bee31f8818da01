"""``zoo.peft`` surface: LoRA adapters on a PatchViT, native to the HIP engine.

The reference reaches this through the Hugging Face ``peft`` package; here the wrapped layer is ``LoraLinear``, whose forward and backward
are ``dinox.ops.lora_linear`` (csrc/lora.hip beside the base ``dinox_gemm``).  The public names, their signatures, the parameter
names inside the model (``...qkv.lora_A.default.weight``) and the files an adapter is stored in (``adapter_config.json``,
``adapter_model.safetensors``) follow what ``peft`` documents, so ``save_adapter`` / ``load_adapter`` keep their meaning.

    model = apply_lora(load_model("ckpt.pth", device="cuda"), rank=8)
    ...train...
    save_adapter(model, "adapter/")
    model = load_adapter(load_model("ckpt.pth", device="cuda"), "adapter/")
    plain = model.merge_and_unload()          # a PatchViT again: fused blocks, adapter folded into fp32 weights

Token, position, patch and scale embeddings describe the scanner's geometry, not the task: ``apply_lora`` never leaves them trainable.
"""
from __future__ import annotations

import json
import logging
import math
from pathlib import Path
from typing import Dict, Iterator, List, Optional, Tuple

import torch
import torch.nn as nn

from dinox import ops
from zoo.arch import PatchViT

log = logging.getLogger(__name__)

__all__ = ["DEFAULT_TARGET_MODULES", "LoraLinear", "LoraModel", "PeftLoraModel", "apply_lora", "save_adapter", "load_adapter",
           "count_parameters"]

DEFAULT_TARGET_MODULES = ["qkv", "proj", "fc1", "fc2"]

ADAPTER = "default"                           # the one adapter name, as in peft's parameter paths
CONFIG_FILE, WEIGHTS_FILE = "adapter_config.json", "adapter_model.safetensors"
MAX_RANK = 64                                 # csrc/lora.hip LORA_MAX_RANK

# substrings of parameter names that stay frozen whatever the caller asks for
_PHYSICAL = ("scale_embed.", "patch_embed.", "cls_token", "pos_embed", "registers")


class LoraLinear(nn.Module):
    """A targeted ``Linear`` with its low-rank side: y = base(x) + (alpha / r) B A dropout(x).  ``lora_A`` / ``lora_B`` are fp32
    ``nn.Linear(bias=False)`` parameter holders in a ``ModuleDict`` keyed by the adapter name; the arithmetic is ``ops.lora_linear``."""

    takes_residual = True                     # zoo.arch hands proj / fc2 the residual stream, the add stays in the product

    def __init__(self, base_layer: nn.Linear, r: int, lora_alpha: float, lora_dropout: float, seed: int = 0) -> None:
        super().__init__()
        if not 1 <= r <= MAX_RANK:
            raise ValueError(f"LoRA rank {r} outside [1, {MAX_RANK}]")
        if not 0.0 <= lora_dropout < 1.0:
            raise ValueError(f"LoRA dropout {lora_dropout} outside [0, 1)")
        self.base_layer = base_layer
        self.in_features, self.out_features = base_layer.in_features, base_layer.out_features
        self.r, self.lora_alpha, self.p = int(r), float(lora_alpha), float(lora_dropout)
        self.scaling = self.lora_alpha / self.r
        kw = dict(bias=False, device=base_layer.weight.device, dtype=torch.float32)
        self.lora_A = nn.ModuleDict({ADAPTER: nn.Linear(self.in_features, self.r, **kw)})
        self.lora_B = nn.ModuleDict({ADAPTER: nn.Linear(self.r, self.out_features, **kw)})
        nn.init.kaiming_uniform_(self.lora_A[ADAPTER].weight, a=math.sqrt(5))
        nn.init.zeros_(self.lora_B[ADAPTER].weight)
        self.merged = False
        self.seed, self.calls = int(seed), 0  # the dropout mask of training call n is a function of (seed, n, element index)

    @property
    def weight(self) -> torch.Tensor:
        return self.base_layer.weight

    @property
    def bias(self) -> Optional[torch.Tensor]:
        return self.base_layer.bias

    def forward(self, x: torch.Tensor, residual: Optional[torch.Tensor] = None, out_dtype=None) -> torch.Tensor:
        base = self.base_layer
        if self.merged:
            return ops.lora_linear(x, base.weight, base.bias, None, None, 0.0, 0.0, None, residual, out_dtype)
        p = self.p if self.training else 0.0
        so = (self.seed, self.calls)
        if p > 0.0:
            self.calls += 1
        return ops.lora_linear(x, base.weight, base.bias, self.lora_A[ADAPTER].weight, self.lora_B[ADAPTER].weight, self.scaling, p, so,
                               residual, out_dtype)

    def _fold(self, sign: int) -> None:
        w = self.base_layer.weight
        new = ops.lora_merge(w.detach(), self.lora_A[ADAPTER].weight, self.lora_B[ADAPTER].weight, self.scaling, sign)
        with torch.no_grad():
            w.copy_(new)                      # through torch, so the cached bf16 images of w see a new version

    def merge(self) -> None:
        if not self.merged:
            self._fold(+1)
            self.merged = True

    def unmerge(self) -> None:
        if self.merged:
            self._fold(-1)
            self.merged = False

    def extra_repr(self) -> str:
        return f"in={self.in_features}, out={self.out_features}, r={self.r}, alpha={self.lora_alpha}, dropout={self.p}"


def _matches(name: str, targets) -> bool:
    return any(name == t or name.endswith("." + t) for t in targets)


def _lora_layers(model: nn.Module) -> Iterator[Tuple[str, LoraLinear]]:
    for name, m in model.named_modules():
        if isinstance(m, LoraLinear):
            yield name, m


def _set_child(root: nn.Module, path: str, new: nn.Module) -> None:
    parent_path, _, leaf = path.rpartition(".")
    setattr(root.get_submodule(parent_path) if parent_path else root, leaf, new)


class LoraModel(nn.Module):
    """Holds the adapted PatchViT as ``.model`` (peft's ``base_model``)."""

    def __init__(self, model: PatchViT) -> None:
        super().__init__()
        self.model = model

    def forward(self, *args, **kwargs):
        return self.model(*args, **kwargs)


class PeftLoraModel(nn.Module):
    """What ``apply_lora`` / ``load_adapter`` return: ``.base_model.model`` is the PatchViT, ``forward(x, spacing=None)`` its forward;
    attributes it does not have itself (``dim``, ``scale_aware``, ``blocks`` ...) are looked up on the PatchViT."""

    def __init__(self, model: PatchViT, config: Dict) -> None:
        super().__init__()
        self.base_model = LoraModel(model)
        self.peft_config = {ADAPTER: dict(config)}

    def __getattr__(self, name: str):
        try:
            return super().__getattr__(name)
        except AttributeError:
            if name == "base_model":
                raise
            return getattr(self.base_model.model, name)

    def forward(self, x: torch.Tensor, spacing: Optional[torch.Tensor] = None) -> torch.Tensor:
        return self.base_model.model(x, spacing=spacing)

    # ---- adapter tensors under peft's on-disk names: the adapter name is left out of the key
    def adapter_state_dict(self) -> Dict[str, torch.Tensor]:
        cfg = self.peft_config[ADAPTER]
        out: Dict[str, torch.Tensor] = {}
        for name, p in self.named_parameters():
            if ".lora_A." in name or ".lora_B." in name:
                out[name.replace(f".{ADAPTER}.", ".")] = p.detach()
        for key, p in self._saved_module_params().items():
            out[key] = p.detach()
        return out

    def _saved_module_params(self) -> Dict[str, torch.Tensor]:
        """On-disk key -> parameter for ``modules_to_save``: ``base_model.model.<module>.modules_to_save.<parameter>``, the key peft
        writes for its wrapper of such a module.  Geometry parameters are frozen whatever the list says and are not stored."""
        cfg, out = self.peft_config[ADAPTER], {}
        for mod_name, m in self.base_model.model.named_modules():
            if mod_name and _matches(mod_name, cfg.get("modules_to_save") or ()):
                for pn, p in m.named_parameters():
                    if not any(tag in f"{mod_name}.{pn}" for tag in _PHYSICAL):
                        out[f"base_model.model.{mod_name}.modules_to_save.{pn}"] = p
        return out

    def save_pretrained(self, save_directory) -> None:
        try:
            from safetensors.torch import save_file
        except ImportError:
            raise ImportError("safetensors is required to store an adapter. Install with: pip install safetensors")
        out = Path(save_directory)
        out.mkdir(parents=True, exist_ok=True)
        if any(m.merged for _, m in _lora_layers(self)):
            raise RuntimeError("the adapter is merged into the base weights: call unmerge_adapter() before saving it")
        (out / CONFIG_FILE).write_text(json.dumps(self.peft_config[ADAPTER], indent=2, sort_keys=True))
        save_file({k: v.cpu().contiguous() for k, v in self.adapter_state_dict().items()}, str(out / WEIGHTS_FILE))

    def merge_adapter(self) -> None:
        for _, m in _lora_layers(self):
            m.merge()

    def unmerge_adapter(self) -> None:
        for _, m in _lora_layers(self):
            m.unmerge()

    def merge_and_unload(self) -> PatchViT:
        """Fold every adapter into its fp32 base weight and put the plain ``Linear`` layers back: the PatchViT's blocks are fusable again."""
        model = self.base_model.model
        for name, m in list(_lora_layers(model)):
            m.merge()
            _set_child(model, name, m.base_layer)
        return model


def _freeze_physical(model: nn.Module) -> int:
    n = 0
    for name, p in model.named_parameters():
        if p.requires_grad and any(tag in name for tag in _PHYSICAL):
            p.requires_grad = False
            n += 1
    return n


def _adapter_config(rank, alpha, target_modules, dropout, modules_to_save, inference_mode=False) -> Dict:
    return {"peft_type": "LORA", "task_type": None, "base_model_name_or_path": None, "r": int(rank), "lora_alpha": float(alpha),
            "lora_dropout": float(dropout), "target_modules": list(target_modules), "bias": "none",
            "modules_to_save": None if modules_to_save is None else list(modules_to_save), "fan_in_fan_out": False,
            "inference_mode": bool(inference_mode), "init_lora_weights": True}


def _inject(model: PatchViT, cfg: Dict) -> PeftLoraModel:
    if not isinstance(model, PatchViT):
        raise TypeError(f"expected a PatchViT, got {type(model).__name__}")
    targets = [(n, m) for n, m in model.named_modules()
               if isinstance(m, nn.Linear) and _matches(n, cfg["target_modules"]) and not any(tag in n + "." for tag in _PHYSICAL)]
    if not targets:
        raise ValueError(f"no nn.Linear of the model matches target_modules={cfg['target_modules']}")
    for p in model.parameters():
        p.requires_grad = False
    seed0 = torch.initial_seed()
    for i, (name, m) in enumerate(targets):
        _set_child(model, name, LoraLinear(m, cfg["r"], cfg["lora_alpha"], cfg["lora_dropout"], seed=seed0 * 1000003 + i))
    for mod_name, m in model.named_modules():
        if mod_name and _matches(mod_name, cfg.get("modules_to_save") or ()):
            for p in m.parameters():
                p.requires_grad = True
    wrapped = PeftLoraModel(model, cfg)
    frozen = _freeze_physical(wrapped)
    if frozen:
        log.info("kept %d geometry parameters frozen", frozen)
    return wrapped


def apply_lora(model: PatchViT, *, rank: int = 8, alpha: float = 16.0, target_modules: Optional[List[str]] = None, dropout: float = 0.05,
               modules_to_save: Optional[List[str]] = None) -> nn.Module:
    """Wrap the targeted ``Linear`` layers of ``model`` (default: qkv, proj, fc1, fc2 of every block) with rank-``rank`` adapters and
    freeze everything else.  ``modules_to_save`` names sub-modules that stay trainable and travel with the adapter -- except the
    geometry layers (scale / patch / position embeddings, CLS and register tokens), which are frozen regardless."""
    cfg = _adapter_config(rank, alpha, DEFAULT_TARGET_MODULES if target_modules is None else target_modules, dropout, modules_to_save)
    wrapped = _inject(model, cfg)
    c = count_parameters(wrapped)
    log.info("LoRA r=%d alpha=%g on %s: %d of %d parameters trainable (%.2f %%)", rank, alpha, cfg["target_modules"], c["trainable"],
             c["total"], 100.0 * c["trainable"] / max(c["total"], 1))
    return wrapped


def save_adapter(model: nn.Module, output_dir) -> Path:
    """Write ``adapter_config.json`` and ``adapter_model.safetensors`` (adapter matrices and ``modules_to_save`` only) to ``output_dir``."""
    out = Path(output_dir)
    out.mkdir(parents=True, exist_ok=True)
    model.save_pretrained(str(out))
    log.info("adapter written to %s", out)
    return out


def load_adapter(model: PatchViT, adapter_path) -> nn.Module:
    """Put a stored adapter onto a base PatchViT.  Like ``peft``'s default the result is for inference: eval mode, nothing trainable."""
    try:
        from safetensors.torch import load_file
    except ImportError:
        raise ImportError("safetensors is required to read an adapter. Install with: pip install safetensors")
    path = Path(adapter_path)
    if not (path / CONFIG_FILE).exists() or not (path / WEIGHTS_FILE).exists():
        raise FileNotFoundError(f"{path} holds no {CONFIG_FILE} / {WEIGHTS_FILE}")
    cfg = json.loads((path / CONFIG_FILE).read_text())
    if cfg.get("peft_type") != "LORA" or cfg.get("bias", "none") != "none":
        raise ValueError(f"{path / CONFIG_FILE}: only LoRA adapters with bias 'none' are supported")
    if isinstance(cfg["target_modules"], str):
        cfg["target_modules"] = [cfg["target_modules"]]
    wrapped = _inject(model, cfg)
    stored = load_file(str(path / WEIGHTS_FILE))
    own = dict(wrapped.named_parameters())
    saved_modules = wrapped._saved_module_params()
    want = set(wrapped.adapter_state_dict())
    if set(stored) != want:
        raise KeyError(f"{path / WEIGHTS_FILE}: missing {sorted(want - set(stored))[:4]}, unexpected {sorted(set(stored) - want)[:4]}")
    with torch.no_grad():
        for key, val in stored.items():
            if key in saved_modules:
                dst = saved_modules[key]
            else:
                dst = own[key.replace(".lora_A.", f".lora_A.{ADAPTER}.").replace(".lora_B.", f".lora_B.{ADAPTER}.")]
            dst.copy_(val.to(dst.device))
    for p in wrapped.parameters():
        p.requires_grad = False
    wrapped.eval()
    log.info("adapter loaded from %s", path)
    return wrapped


def count_parameters(model: nn.Module) -> Dict[str, int]:
    """{"total", "trainable", "frozen"} element counts."""
    total = sum(p.numel() for p in model.parameters())
    trainable = sum(p.numel() for p in model.parameters() if p.requires_grad)
    return {"total": total, "trainable": trainable, "frozen": total - trainable}
