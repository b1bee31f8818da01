"""CPU checks of the segmentation path: the float64 oracle (tests/_segloss_oracle.py) against the framework statement people mean
(F.interpolate bilinear + F.cross_entropy(ignore_index=255) + the Dice formula under autograd, float64), the paired image / mask
transforms, the metric helpers, and the command line of scripts/finetune_segmentation.py."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _segloss_oracle as SO
from conftest import ROOT


def torch_statement(z, y, g, u, w_ce, w_dice, c0):
    """-> (loss[3], stats[3, C], dz) in float64 by framework code."""
    z = torch.from_numpy(z).double().requires_grad_(True)
    yt = torch.from_numpy(y.astype(np.int64))
    B, P, C = z.shape
    logits = F.interpolate(z.reshape(B, g, g, C).permute(0, 3, 1, 2), scale_factor=u, mode="bilinear", align_corners=False)
    valid = (yt != 255)
    if not valid.any():
        return None
    ce = F.cross_entropy(logits, yt, ignore_index=255)
    p = logits.softmax(1) * valid[:, None]
    oh = torch.stack([(yt == c) & valid for c in range(C)], 1).double()
    I, Pc, Y = (p * oh).sum((0, 2, 3)), p.sum((0, 2, 3)), oh.sum((0, 2, 3))
    D = (2 * I + 1) / (Pc + Y + 1)
    dice = 1 - D[c0:].mean()
    L = w_ce * ce + w_dice * dice
    L.backward()
    return (torch.stack([L, ce, dice]).detach().numpy(), torch.stack([I, Pc, Y]).detach().numpy(), z.grad.numpy())


def labels(rng, B, S, C, ignore=0.25):
    y = rng.integers(0, C, (B, S, S)).astype(np.uint8)
    y[rng.random((B, S, S)) < ignore] = 255
    return y


@pytest.mark.parametrize("g,u", [(1, 4), (2, 3), (3, 16), (5, 7), (14, 16)])
@pytest.mark.parametrize("C,c0,w_ce,w_dice", [(2, 0, 1.0, 1.0), (5, 1, 0.7, 1.3), (33, 1, 0.0, 1.0), (7, 0, 1.0, 0.0)])
def test_oracle_is_the_framework_statement(g, u, C, c0, w_ce, w_dice):
    B = 1 if g == 14 else 3
    rng = np.random.default_rng([g, u, C])
    z = rng.standard_normal((B, g * g, C)) * 3
    y = labels(rng, B, g * u, C)
    want = torch_statement(z, y, g, u, w_ce, w_dice, c0)
    fwd = SO.forward(z, y, g, u, w_ce, w_dice, c0)
    dz, _ = SO.backward(z, y, g, u, w_ce, w_dice, c0)
    for got, ref in ((fwd["loss"], want[0]), (fwd["stats"], want[1]), (dz, want[2])):
        assert np.abs(got - ref).max() <= 1e-10 * max(np.abs(ref).max(), 1e-300)
    two = SO.backward(z, y, g, u, w_ce, w_dice, c0, grad_scale=-2.5)[0]
    assert np.abs(two + 2.5 * want[2]).max() <= 1e-10 * np.abs(want[2]).max()


def test_oracle_all_ignored_is_zero():
    rng = np.random.default_rng(3)
    z = rng.standard_normal((2, 4, 3))
    y = np.full((2, 6, 6), 255, dtype=np.uint8)
    fwd = SO.forward(z, y, 2, 3)
    assert fwd["nv"] == 0 and not fwd["loss"].any() and not SO.backward(z, y, 2, 3)[0].any()


def test_oracle_bounds_are_small_and_positive():
    rng = np.random.default_rng(4)
    z = rng.standard_normal((2, 9, 5))
    y = labels(rng, 2, 48, 5)
    fwd = SO.forward(z, y, 3, 16)
    dz, e = SO.backward(z, y, 3, 16)
    # 4608 pixels feed the sums: n u = 2.7e-4 relative on losses of order 1, and on a gradient that is a mean over those pixels
    assert (fwd["e_loss"] > 0).all() and (fwd["e_loss"] < 2e-3).all() and (e > 0).all() and (e < 2e-3 * np.abs(dz).max()).all()


def test_oracle_predict_and_counts():
    z = np.zeros((1, 4, 3))
    z[0, :, 1] = [1.0, -1.0, -1.0, 1.0]                     # class 1 wins around patches 0 and 3, an exact tie 0 / 2 elsewhere -> 0
    pred, margin, e_l = SO.predict(z, 2, 2)
    assert pred[0, 0, 0] == 1 and pred[0, 0, 3] == 0 and pred[0, 3, 3] == 1 and (e_l >= 0).all() and margin[0, 0, 0] == 1.0
    y = np.array([[[1, 1, 0, 255], [1, 1, 0, 0], [0, 0, 1, 1], [2, 0, 1, 1]]], dtype=np.uint8)
    c = SO.counts(pred, y, 3)
    assert c[2].tolist() == [6, 8, 1] and c[:, 2].tolist() == [0, 0, 1] and c[1].sum() == 15


# ------------------------------------------------------------------------------------------ dinox.segment metric helpers
def test_metric_helpers_on_hand_made_counts():
    from dinox import segment as SG
    counts = torch.tensor([[8, 3, 0, 0], [10, 5, 2, 0], [9, 6, 0, 2]])         # tp, predicted, labelled; class 3 is never predicted
    d = SG.dice_per_class(counts)
    assert d.tolist() == pytest.approx([16 / 19, 6 / 11, 0.0, 0.0])
    assert SG.mean_dice(counts) == pytest.approx((16 / 19 + 6 / 11 + 0.0 + 0.0) / 4)
    assert SG.mean_dice(counts, skip_background=True) == pytest.approx((6 / 11 + 0.0 + 0.0) / 3)
    assert SG.miou(counts) == pytest.approx((8 / 11 + 3 / 8 + 0.0 + 0.0) / 4)
    assert SG.pixel_accuracy(counts) == pytest.approx(11 / 17)
    empty = torch.zeros((3, 2), dtype=torch.int64)                              # nothing valid: no division by zero
    assert SG.mean_dice(empty) == 0.0 and SG.miou(empty) == 0.0 and SG.pixel_accuracy(empty) == 0.0
    absent = torch.tensor([[4, 0], [4, 0], [4, 0]])                             # a class in neither map is left out of the means
    assert SG.mean_dice(absent) == 1.0 and SG.miou(absent) == 1.0


# ------------------------------------------------------------------------------------------ scripts/finetune_segmentation.py
def _script():
    if "finetune_segmentation" in sys.modules:
        return sys.modules["finetune_segmentation"]
    spec = importlib.util.spec_from_file_location("finetune_segmentation", os.path.join(ROOT, "dino-x_amd", "scripts", "finetune_segmentation.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


SHARED = ["backbone", "device", "train_csv", "val_csv", "synthetic", "data_root", "input_format", "window_level", "window_width", "num_classes",
          "rank", "alpha", "lora_dropout", "epochs", "batch_size", "lr", "weight_decay", "warmup_epochs", "patience", "es_metric", "num_workers",
          "no_amp", "seed", "unfreeze_blocks", "backbone_lr", "output"]


def test_parser_flags_and_defaults():
    fs = _script()
    import finetune_lora as fl
    mine = {a.dest: a for a in fs.build_parser()._actions if a.dest != "help"}
    base = {a.dest: a for a in fl.build_parser()._actions if a.dest != "help"}
    assert set(mine) == set(SHARED) | {"ce_weight", "dice_weight", "dice_skip_background", "ignore_index"}
    for k in SHARED:
        if k != "es_metric":
            assert mine[k].default == base[k].default and mine[k].required == base[k].required, k
    a = fs.build_parser().parse_args(["--backbone", "b", "--output", "o"])
    assert (a.ce_weight, a.dice_weight, a.dice_skip_background, a.ignore_index, a.es_metric) == (1.0, 1.0, False, 255, "loss")
    assert fs.build_parser().parse_args(["--backbone", "b", "--output", "o", "--es-metric", "mean_dice"]).es_metric == "mean_dice"
    with pytest.raises(SystemExit):
        fs.build_parser().parse_args(["--backbone", "b", "--output", "o", "--es-metric", "auroc"])


@pytest.mark.parametrize("extra,what", [(["--ignore-index", "0"], "ignore-index"), (["--num-classes", "65"], "num-classes"),
                                         (["--num-classes", "1"], "num-classes")])
def test_script_refusals(extra, what, capsys):
    fs = _script()
    args = fs.build_parser().parse_args(["--backbone", "nowhere", "--output", "o", "--synthetic", "8", *extra])
    with pytest.raises(SystemExit):
        fs.run(args)                                        # refused before the backbone is looked for
    assert what in capsys.readouterr().err


def test_paired_transforms_move_image_and_mask_together():
    fs = _script()
    S = 40
    yy, xx = torch.meshgrid(torch.arange(S), torch.arange(S), indexing="ij")
    mask = ((yy // 10) * 4 + xx // 10).to(torch.uint8) * 3            # 16 blocks with the values 0, 3, ..., 45
    mask[:, :2] = 255
    img = (mask.float() / 255.0)[None].expand(3, -1, -1)              # the image IS the mask: whatever window the pair gets, they must agree
    src = set(mask.unique().tolist())
    gen = torch.Generator().manual_seed(5)
    flips = 0
    for _ in range(12):
        x, m = fs.paired_transform(img, mask, 32, gen, augment=True)
        assert x.shape == (3, 32, 32) and m.shape == (32, 32) and m.dtype == torch.uint8
        assert set(m.unique().tolist()) <= src                        # nearest: only values that were in the source mask
        back = x[0] * 0.229 + 0.485                                   # undo the normalisation of channel 0
        inner = (m == m.roll(1, 0)) & (m == m.roll(-1, 0)) & (m == m.roll(1, 1)) & (m == m.roll(-1, 1))
        inner[0], inner[-1], inner[:, 0], inner[:, -1] = False, False, False, False
        assert inner.sum() > 100
        assert (back[inner] - m[inner].float() / 255.0).abs().max() < 0.08     # away from the block edges bicubic ringing is small
        flips += int(m[:, -3:].eq(255).any())                         # the ignore strip moved to the right edge: the flip hit both
    assert 0 < flips < 12
    x, m = fs.paired_transform(img, mask, 32, gen, augment=False)      # validation: the centre crop for both, no randomness
    x2, m2 = fs.paired_transform(img, mask, 32, gen, augment=False)
    assert torch.equal(x, x2) and torch.equal(m, m2) and set(m.unique().tolist()) <= src
