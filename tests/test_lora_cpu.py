"""CPU checks of the LoRA feature: the C-ABI entries (declared, exported, argument checks before any launch), zoo.peft's bookkeeping on a
CPU-constructed PatchViT, the adapter files, the metrics and the flag surface of scripts/finetune_lora.py, and the dropout hash."""
import ctypes
import importlib.util
import json
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

import _lora_oracle as LO
from conftest import ROOT

ENTRIES = ("dinox_lora_down", "dinox_lora_up", "dinox_lora_grad_ws_bytes", "dinox_lora_grad", "dinox_lora_dropout", "dinox_lora_merge")
TINY = dict(img_size=32, patch=8, dim=32, depth=2, heads=2, scale_aware=True)


@pytest.fixture(scope="module")
def ft():
    spec = importlib.util.spec_from_file_location("finetune_lora", os.path.join(ROOT, "dino-x_amd", "scripts", "finetune_lora.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------------------------------ C ABI
def test_entries_declared_exported_and_bound():
    from dinox import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dinox.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        m = re.search(r"\b(?:int|int64_t)\s+" + name + r"\s*\(([^;{]*?)\)\s*;", header, flags=re.S)
        assert m, f"{name} is not declared in dinox.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert len(_lib.SIGNATURES[name][1]) == len([a for a in m.group(1).split(",") if a.strip()])
    assert _lib.lib.dinox_version() == 3


def test_entries_reject_bad_arguments_before_any_launch():
    """No GPU here: a call that got as far as a launch would fail with a HIP error code, not with -1 and these messages."""
    from dinox import _lib
    L = _lib.lib
    a = ctypes.create_string_buffer(64)
    p = ctypes.addressof(a)

    def bad(rc, word):
        assert rc == -1 and word in _lib.last_error(), (rc, _lib.last_error())

    bad(L.dinox_lora_down(None, p, p, 4, 8, 2, 0, 0, None), "null pointer")
    bad(L.dinox_lora_up(p, None, None, p, 1.0, 4, 8, 2, 0, None), "null pointer")
    bad(L.dinox_lora_grad(p, p, p, p, 1.0, p, p, None, 4, 8, 8, 2, 0, None), "null pointer")
    bad(L.dinox_lora_dropout(None, p, 4, 0.5, 1, 2, 0, None), "null pointer")
    bad(L.dinox_lora_merge(p, p, p, None, 1.0, 1, 4, 4, 2, None), "null pointer")
    for r in (0, 65, 66, -1):
        bad(L.dinox_lora_down(p, p, p, 4, 8, r, 0, 0, None), "r=")
        bad(L.dinox_lora_up(p, p, None, p, 1.0, 4, 8, r, 0, None), "r=")
        bad(L.dinox_lora_grad(p, p, p, p, 1.0, p, p, p, 4, 8, 8, r, 0, None), "r=")
        bad(L.dinox_lora_merge(p, p, p, p, 1.0, 1, 4, 4, r, None), "r=")
        assert L.dinox_lora_grad_ws_bytes(4, 8, 8, r) == 0
    bad(L.dinox_lora_down(p, p, p, 0, 8, 2, 0, 0, None), "M=0")
    bad(L.dinox_lora_up(p, p, None, p, 1.0, 0, 8, 2, 0, None), "M=0")
    bad(L.dinox_lora_grad(p, p, p, p, 1.0, p, p, p, 0, 8, 8, 2, 0, None), "M=0")
    bad(L.dinox_lora_down(p, p, p, 4, 0, 2, 0, 0, None), "K=0")
    bad(L.dinox_lora_down(p, p, p, 4, 8, 2, 2, 0, None), "small_layout")
    bad(L.dinox_lora_down(p, p, p, 4, 8, 2, 0, 7, None), "dtype")
    bad(L.dinox_lora_merge(p, p, p, p, 1.0, 0, 4, 4, 2, None), "sign")
    for prob in (-0.1, 1.0, 1.5, float("nan")):
        bad(L.dinox_lora_dropout(p, p, 4, prob, 1, 2, 0, None), "outside [0, 1)")
    bad(L.dinox_lora_dropout(p, p, 0, 0.5, 1, 2, 0, None), "n=0")
    assert L.dinox_lora_grad_ws_bytes(130, 36, 20, 4) == 2 * (4 * 36 + 20 * 4) * 4


# ------------------------------------------------------------------------------------------ zoo.peft bookkeeping
def _vit():
    import zoo.arch as arch
    torch.manual_seed(0)
    return arch.PatchViT(**TINY)


def test_apply_lora_trains_the_adapter_only():
    from zoo.peft import DEFAULT_TARGET_MODULES, LoraLinear, apply_lora, count_parameters
    assert DEFAULT_TARGET_MODULES == ["qkv", "proj", "fc1", "fc2"]
    vit = _vit()
    n_base = sum(p.numel() for p in vit.parameters())
    w = apply_lora(vit, rank=4)
    assert w.base_model.model is vit and w.dim == 32
    trainable = {k for k, p in w.named_parameters() if p.requires_grad}
    assert trainable and all(".lora_A.default.weight" in k or ".lora_B.default.weight" in k for k in trainable)
    assert len(trainable) == 2 * 4 * 2
    n_lora = 2 * (4 * (32 + 96) + 4 * (32 + 32) + 4 * (32 + 128) + 4 * (128 + 32))
    assert count_parameters(w) == {"total": n_base + n_lora, "trainable": n_lora, "frozen": n_base}
    keys = set(w.state_dict())
    for leaf in ("attn.qkv", "attn.proj", "mlp.fc1", "mlp.fc2"):
        for tail in ("base_layer.weight", "base_layer.bias", "lora_A.default.weight", "lora_B.default.weight"):
            assert f"base_model.model.blocks.1.{leaf}.{tail}" in keys
    lay = vit.blocks[0].attn.qkv
    assert isinstance(lay, LoraLinear) and lay.lora_A["default"].weight.shape == (4, 32) and lay.lora_B["default"].weight.shape == (96, 4)
    assert lay.scaling == 16.0 / 4 and lay.p == 0.05 and not lay.lora_B["default"].weight.any()
    bound = 1.0 / math.sqrt(32)                                   # kaiming-uniform with a = sqrt(5): U(-1/sqrt(fan_in), 1/sqrt(fan_in))
    a = lay.lora_A["default"].weight
    assert a.abs().max() <= bound and a.abs().max() > 0.5 * bound
    assert not any(b._fusable() for b in vit.blocks)
    with pytest.raises(ValueError):
        apply_lora(_vit(), rank=65)
    with pytest.raises(ValueError):
        apply_lora(_vit(), rank=4, target_modules=["nothing"])


def test_modules_to_save_and_the_geometry_freeze():
    from zoo.peft import apply_lora
    w = apply_lora(_vit(), rank=2, target_modules=["qkv"], modules_to_save=["norm", "scale_embed", "patch_embed"])
    trainable = {k for k, p in w.named_parameters() if p.requires_grad}
    assert {"base_model.model.norm.weight", "base_model.model.norm.bias"} <= trainable
    assert not any(tag in k for k in trainable for tag in ("scale_embed.", "patch_embed.", "cls_token", "pos_embed", "registers"))
    assert all(".lora_" in k or ".norm." in k for k in trainable)
    assert not any(".proj.lora_" in k for k in trainable)


def test_adapter_round_trip_is_bit_exact(tmp_path):
    from safetensors.torch import load_file
    from zoo.peft import apply_lora, load_adapter, save_adapter
    w = apply_lora(_vit(), rank=4, alpha=8.0, dropout=0.1, modules_to_save=["norm", "patch_embed"])      # geometry: frozen, never stored
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for k, p in w.named_parameters():
            if ".lora_B." in k or ".norm." in k:
                p.copy_(torch.randn(p.shape, generator=g))
    assert save_adapter(w, tmp_path / "a") == tmp_path / "a"
    cfg = json.loads((tmp_path / "a" / "adapter_config.json").read_text())
    assert (cfg["peft_type"], cfg["r"], cfg["lora_alpha"], cfg["lora_dropout"], cfg["bias"]) == ("LORA", 4, 8.0, 0.1, "none")
    assert cfg["target_modules"] == ["qkv", "proj", "fc1", "fc2"] and cfg["modules_to_save"] == ["norm", "patch_embed"]
    stored = load_file(str(tmp_path / "a" / "adapter_model.safetensors"))
    want = {f"base_model.model.blocks.{i}.{leaf}.lora_{ab}.weight" for i in range(2) for leaf in ("attn.qkv", "attn.proj", "mlp.fc1", "mlp.fc2")
            for ab in "AB"} | {"base_model.model.norm.modules_to_save.weight", "base_model.model.norm.modules_to_save.bias"}
    assert set(stored) == want
    w2 = load_adapter(_vit(), tmp_path / "a")
    assert w2.peft_config["default"] == cfg and not w2.training and not any(p.requires_grad for p in w2.parameters())
    a, b = w.state_dict(), w2.state_dict()
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    with pytest.raises(FileNotFoundError):
        load_adapter(_vit(), tmp_path / "missing")


# ------------------------------------------------------------------------------------------ metrics and flags
def test_auroc_against_sklearn_and_by_hand(ft):
    from sklearn.metrics import roc_auc_score
    rng = np.random.default_rng(0)
    for n, levels in ((50, None), (200, 7), (31, 2)):
        y = rng.integers(0, 2, n)
        s = rng.standard_normal(n) + y if levels is None else rng.integers(0, levels, n).astype(np.float64) + 0.5 * y
        assert ft.auroc(torch.from_numpy(s), torch.from_numpy(y)) == pytest.approx(roc_auc_score(y, s), abs=1e-12)
    assert ft.auroc(torch.tensor([0.5, 0.5, 0.5, 0.5]), torch.tensor([0, 1, 0, 1])) == 0.5           # all tied
    assert ft.auroc(torch.tensor([0.1, 0.4, 0.4, 0.8]), torch.tensor([0, 0, 1, 1])) == 0.875          # one tie across the classes
    assert ft.auroc(torch.tensor([0.1, 0.9]), torch.tensor([1, 1])) == 0.5                             # a single class


def test_compute_metrics_by_hand(ft):
    logits = torch.tensor([[2.0, 0.0], [0.0, 1.0], [1.0, 0.0], [0.0, 3.0]])
    m = ft.compute_metrics(logits, torch.tensor([0, 1, 1, 1]), "classification", 2)
    assert m["accuracy"] == 0.75 and m["auroc"] == 1.0          # the one negative has the lowest class-1 score
    assert m["macro_f1"] == pytest.approx((2 / 3 + 0.8) / 2, abs=1e-6)           # class 0: p 1/2, r 1; class 1: p 1, r 2/3
    one = ft.compute_metrics(logits, torch.tensor([1, 1, 1, 1]), "classification", 2)
    assert one["auroc"] == 0.5 and one["accuracy"] == 0.5 and one["macro_f1"] == pytest.approx(2 / 3, abs=1e-6)
    three = ft.compute_metrics(torch.eye(3), torch.tensor([0, 1, 2]), "classification", 3)
    assert three == {"accuracy": 1.0, "macro_f1": pytest.approx(1.0, abs=1e-6)}
    r = ft.compute_metrics(torch.tensor([[1.0], [2.0], [4.0]]), torch.tensor([1.0, 2.0, 3.0]), "regression", 1)
    assert r["mse"] == pytest.approx(1 / 3) and r["rmse"] == pytest.approx(math.sqrt(1 / 3)) and r["r2"] == pytest.approx(0.5)
    const = ft.compute_metrics(torch.tensor([[1.0], [3.0]]), torch.tensor([2.0, 2.0]), "regression", 1)
    assert const["r2"] == 0.0 and const["mse"] == 1.0


def test_parser_defaults(ft):
    ap = ft.build_parser()
    a = ap.parse_args(["--backbone", "b", "--output", "o"])
    want = dict(train_csv=None, val_csv=None, data_root=None, input_format="hu16_png", window_level=40.0, window_width=400.0,
                task="classification", num_classes=2, rank=8, alpha=16.0, lora_dropout=0.05, epochs=50, batch_size=32, lr=1e-3,
                weight_decay=0.01, warmup_epochs=3, patience=10, es_metric="loss", num_workers=4, no_amp=False, seed=None,
                unfreeze_blocks=0, backbone_lr=1e-5, synthetic=0)
    for k, v in want.items():
        assert getattr(a, k) == v, k
    with pytest.raises(SystemExit):
        ap.parse_args(["--output", "o"])                               # --backbone is required


def test_synthetic_labels_can_be_read_off_the_pixels(ft):
    ds = ft.SyntheticStacks(16, 32, "classification", 2, seed=0)
    for i in range(16):
        x, sp, y = ds[i]
        assert x.shape == (3, 32, 32) and sp.shape == (3,)
        assert (x[:, :16].mean() > x[:, 16:].mean()) == (y == 1.0)
    again = ft.SyntheticStacks(16, 32, "classification", 2, seed=0)
    assert torch.equal(ds[3][0], again[3][0])
    x = torch.rand(3, 40, 60)
    assert ft.resize_center_crop(x, 32).shape == (3, 32, 32)
    assert ft.random_resized_crop(x, 32, torch.Generator().manual_seed(0)).shape == (3, 32, 32)


# ------------------------------------------------------------------------------------------ dropout hash
@pytest.mark.parametrize("p", (0.05, 0.5))
def test_keep_rate_of_the_hash(p):
    n = 1 << 16
    for seed, offset in ((0, 0), (12345, 7), (2 ** 40 + 3, 2 ** 35)):
        kept = int(LO.keep_mask(n, p, seed, offset).sum())
        sd = math.sqrt(n * p * (1 - p))
        assert abs(kept - n * (1 - p)) <= 4.5 * sd, (p, seed, offset, kept)          # 4.5 sigma: 7e-6 per draw under a fair hash
    assert LO.keep_mask(64, 0.0, 1, 2).all()
    assert not np.array_equal(LO.keep_mask(n, p, 1, 0), LO.keep_mask(n, p, 1, 1))    # another call, another mask
    assert np.array_equal(LO.keep_mask(100, p, 1, 1, start=50), LO.keep_mask(150, p, 1, 1)[50:])
