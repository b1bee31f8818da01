"""GPU tests of patch-based training at native resolution: csrc/segpatch.hip through ops.seg_patch_sample against the float64 oracle and
the fp32 emulation of tests/_segpatch_oracle.py on the seeded launches of tests/_segpatch_cases.py, and
scripts/finetune_segmentation.py --patch-train end to end on a tiny backbone.

Every launch reads a poisoned pool (NaN and 0xAB guard elements around every plane, odd offsets) and writes into outputs with guard
elements around them, the label batch at an odd byte offset in half of the launches (so both label store paths run).  x is held to the
derived bound at every pixel; m equals the fp32 emulation at every pixel and the float64 oracle outside the band in which an integer
lies within delta of a coordinate.  The largest share of a job's pixels in that band is 0.0002 (tests/test_segpatch_cpu.py computes it
from the oracle alone; the cap is 0.01).  Jobs with gamma != 1 carry the powf term at twice the recorded error (POW_ULP_RECORDED);
jobs with gamma == 1 are held to the derived bound alone."""
import importlib.util
import json
import os
import sys

import numpy as np
import pytest
import torch

import _segpatch_cases as K
import _segpatch_oracle as O
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD_X, GUARD_M = 12345.0, 0x5C


@pytest.fixture(scope="module")
def pools():
    _, img, msk, _, _ = K.pool()
    return torch.from_numpy(img.copy()).to(DEV), torch.from_numpy(msk.copy()).to(DEV)


def _guarded(B, S, odd):
    """Output tensors that are views into larger buffers filled with guard values: (x, m, xbuf, mbuf, x offset, m offset)."""
    nx, nm, ox, om = B * 3 * S * S, B * S * S, 7, 5 if odd else 8
    xbuf = torch.full((nx + 2 * ox,), GUARD_X, dtype=torch.float32, device=DEV)
    mbuf = torch.full((nm + 16,), GUARD_M, dtype=torch.uint8, device=DEV)
    return xbuf[ox:ox + nx].view(B, 3, S, S), mbuf[om:om + nm].view(B, S, S), xbuf, mbuf, ox, om


def _run(pools, c, mean=K.MEAN, std=K.STD, odd=False):
    from dinox import ops
    x, m, xbuf, mbuf, ox, om = _guarded(c["B"], c["S"], odd)
    gx, gm = ops.seg_patch_sample(pools[0], pools[1], c["jobs"], c["par"], c["S"], mean, std, c["pad"], out=(x, m))
    assert gx.data_ptr() == x.data_ptr() and gm.data_ptr() == m.data_ptr()
    xb, mb = xbuf.cpu().numpy(), mbuf.cpu().numpy()
    assert (xb[:ox] == GUARD_X).all() and (xb[ox + x.numel():] == GUARD_X).all(), "a store left x"
    assert (mb[:om] == GUARD_M).all() and (mb[om + m.numel():] == GUARD_M).all(), "a store left m"
    return x.cpu().numpy(), m.cpu().numpy()


@pytest.mark.parametrize("i", range(len(K.LAUNCHES)))
def test_launch_equals_the_oracle(pools, i):
    from dinox import ops
    c = K.launch(i)
    x, m = _run(pools, c, odd=bool(i % 2))
    _, m32 = O.emulate32(K.pool()[0], c["plane_of"], c["par"], c["S"], K.MEAN, K.STD, c["pad"])
    ratio, share = c["want"].check(x, m, m32)
    print(f"launch {i} S={c['S']} B={c['B']} kinds {c['kinds'][0]}..: error / bound {ratio:.3f}, band share {share:.5f}")
    for b, kind in enumerate(c["kinds"]):
        if kind == "far":                                   # a centre far outside: every label 255, every value (pad - mean) / std to the bit
            assert (m[b] == 255).all()
            for ch in range(3):
                assert (x[b, ch] == (np.float32(c["pad"]) - np.float32(K.MEAN[ch])) / np.float32(K.STD[ch])).all()
    # the allocating call and a second launch: equal bytes
    x2, m2 = ops.seg_patch_sample(pools[0], pools[1], c["jobs"], c["par"], c["S"], K.MEAN, K.STD, c["pad"])
    assert x2.dtype == torch.float32 and m2.dtype == torch.uint8 and tuple(x2.shape) == (c["B"], 3, c["S"], c["S"]) and tuple(m2.shape) == (c["B"], c["S"], c["S"])
    assert np.array_equal(x2.cpu().numpy().view(np.uint32), x.view(np.uint32)) and np.array_equal(m2.cpu().numpy(), m)
    # the pool is untouched, guards included
    _, img, msk, _, _ = K.pool()
    assert np.array_equal(pools[0].cpu().numpy().view(np.uint32), img.view(np.uint32)) and np.array_equal(pools[1].cpu().numpy(), msk)


def test_exact_jobs_are_exact(pools):
    """Identity, integer shift, mirrors and quarter turns at mean 0, std 1: x is the plane's own bits (or pad), m its labels."""
    _, _, _, oi, om = K.pool()
    img, msk = K.pool()[0][2]
    S = 28
    kinds = ["identity", "shift", "mirror_x", "mirror_y", "turn1", "turn2", "turn3"]
    par = np.stack([K.job_par(k, 64, 64, S, None) for k in kinds])
    c = dict(S=S, B=len(kinds), jobs=np.array([[oi[2], om[2], 64, 64]] * len(kinds), dtype=np.int64), par=par, pad=0.0)
    x, m = _run(pools, c, mean=(0, 0, 0), std=(1, 1, 1))
    x32, m32 = O.emulate32(K.pool()[0], [2] * len(kinds), par, S, (0, 0, 0), (1, 1, 1), 0.0)
    assert np.array_equal(x.view(np.uint32), x32.view(np.uint32)) and np.array_equal(m, m32)
    assert np.array_equal(x[0, 1], img[:S, :S]) and np.array_equal(m[0], msk[:S, :S])
    assert np.array_equal(x[2, 0], img[:S, :S][:, ::-1]) and np.array_equal(m[3], msk[:S, :S][::-1])


def test_pow_error_is_within_twice_the_record(pools):
    """powf is the one operation whose accuracy this code base cannot derive: the error of gain * v^gamma against float64, in units of
    u |exact|, on integer-shift jobs at mean 0, std 1 (so v is a plane value and x is v' itself).  Recorded on the MI355X:
    POW_ULP_RECORDED (tests/_segpatch_oracle.py); gated at twice that."""
    c = K.pow_launch()
    x, _ = _run(pools, c, mean=(0, 0, 0), std=(1, 1, 1))
    want = O.sample64(K.pool()[0], c["plane_of"], c["par"], c["S"], (0, 0, 0), (1, 1, 1), 0.0)
    inside = want.m != 255                                   # (a mask value of 255 inside the plane only drops a pixel from the measurement)
    err = np.abs(x[:, 0].astype(np.float64) - want.vprime) / (O.U * np.abs(want.vprime))
    worst = float(err[inside & (want.vprime > 0)].max())
    print(f"largest error of gain * powf(v, gamma): {worst:.3f} u (recorded {O.POW_ULP_RECORDED}, gate {O.POW_ULP})")
    assert worst <= O.POW_ULP
    assert (x[:, 0][~inside & (np.abs(want.vprime) == 0)] == 0).all()


# ------------------------------------------------------------------------------------------ end to end on a tiny backbone
TINY = dict(img_size=32, patch=8, dim=32, depth=2, heads=2, scale_aware=True)      # the configuration tests/test_segblend_gpu.py builds
# train_loss_history of _argv() without --patch-train on the commit before patch training (MI355X)
PARENT_HISTORY = [1.7785550753275554, 1.511011044184367]


def _script():
    if "finetune_segmentation" in sys.modules:
        return sys.modules["finetune_segmentation"]
    spec = importlib.util.spec_from_file_location("finetune_segmentation", os.path.join(ROOT, "dino-x_amd", "scripts", "finetune_segmentation.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def backbone_dir(tmp_path_factory):
    import zoo.arch as arch
    from zoo.hub import export_hub_checkpoint
    torch.manual_seed(0)
    m = arch.PatchViT(**TINY)
    with torch.no_grad():
        m.scale_embed.mlp[2].weight.normal_(0, 0.05)
    d = tmp_path_factory.mktemp("tiny_hub_patch")
    export_hub_checkpoint(m.to(DEV).eval(), d, config=dict(TINY, mlp_ratio=4.0, num_registers=4))
    return d


def _argv(backbone_dir, out, *more):
    return ["--backbone", str(backbone_dir), "--synthetic", "24", "--num-classes", "3", "--epochs", "2", "--batch-size", "6", "--lr", "1e-2",
            "--seed", "0", "--no-amp", "--output", str(out), *more]


def test_patch_training_end_to_end(backbone_dir, tmp_path):
    from dinox.segment import load_segmenter, segment_tiled
    fs = _script()
    flags = ("--rank", "0", "--patch-train", "--patch-val", "tiled", "--patch-size", "24", "--patches-per-epoch", "36")
    res = fs.run(fs.parse_cli(_argv(backbone_dir, tmp_path / "a", *flags)))
    cfg = res["config"]
    print(f"patch training: train loss per epoch {cfg.train_loss_history}, best validation metrics {cfg.best_val_metrics}")
    assert len(cfg.train_loss_history) == 2 and all(np.isfinite(cfg.train_loss_history)) and np.isfinite(cfg.best_val_loss)
    assert {"seg_head.pth", "finetune_config.json"} == {p.name for p in (tmp_path / "a").iterdir()}
    saved = json.loads((tmp_path / "a" / "finetune_config.json").read_text())
    assert (saved["patch_train"], saved["patch_size"], saved["patch_fg_prob"], saved["patch_rotate_deg"], saved["patch_scale"], saved["patches_per_epoch"],
            saved["patch_val"]) == (True, 24, 0.33, 15.0, [0.7, 1.4], 36, "tiled")
    assert len(res["val_pred"]) == 6 and all(p.shape == (32, 32) and p.dtype == np.uint8 for p in res["val_pred"])
    model = load_segmenter(backbone_dir, tmp_path / "a", DEV)
    ds = res["val_dataset"]
    sx, sy, sz = ds.spacings[0].tolist()
    got = segment_tiled(model, ds.images[0, 0].numpy(), (sx, sy), sz, tile=24, input_format="windowed_float")
    assert got.shape == (32, 32) and np.array_equal(got, res["val_pred"][0])      # what the run's tiled validation labelled (fp32 both times)
    again = fs.run(fs.parse_cli(_argv(backbone_dir, tmp_path / "b", *flags)))["config"]
    assert again.train_loss_history == cfg.train_loss_history and again.best_val_metrics == cfg.best_val_metrics


def test_without_the_flag_nothing_changed(backbone_dir, tmp_path):
    from dinox.segment import load_segmenter
    fs = _script()
    new = fs.run(fs.parse_cli(_argv(backbone_dir, tmp_path / "a")))["config"]
    old_style = fs.run(fs.build_parser().parse_args(_argv(backbone_dir, tmp_path / "b")))["config"]       # a namespace without the patch attributes
    print(f"without --patch-train: train loss per epoch {new.train_loss_history!r}")
    assert new.train_loss_history == old_style.train_loss_history and not new.patch_train and new.patch_val == "center"
    assert new.train_loss_history == PARENT_HISTORY
    cfg = json.loads((tmp_path / "a" / "finetune_config.json").read_text())
    for k in [k for k in cfg if k.startswith("patch")]:      # a config file from before patch training has none of these keys: it loads alike
        del cfg[k]
    (tmp_path / "a" / "finetune_config.json").write_text(json.dumps(cfg))
    assert not load_segmenter(backbone_dir, tmp_path / "a", DEV).training
