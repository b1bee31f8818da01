"""GPU tests of the edge-aware refinement: csrc/segrefine.hip through ops.seg_refine against the float64 oracle
(tests/_segrefine_oracle.py) within its a-priori bounds -- pred on every decided pixel, conf within its bound there, counts integer for
integer against the recount from the returned map --, T = 0 bit for bit ops.seg_predict / ops.seg_calib, w = 0, lambda = 0 and a
constant guide, determinism, non-finite inputs, batch independence, and dinox.segment / the scripts end to end.

Shapes: the calibration set -- (1, 4), (2, 3), (3, 16), (5, 1), (2, 32), (14, 16); B = 1, 3; C = 2, 5, 33, 64.  Every (g, u, B, C) runs
the cases of tests/test_segrefine_cpu.py (``gpu_cases`` / ``case_params``): T, (r, d), lambda, w, s, the sigmas, the logit and label
regimes of tests/test_segloss_gpu.py and the alignment of z and the guide cycle through them.  A case whose r d reaches across the image
(or whose 2 d > S would leave the middle pixels no neighbour) is not run: its refusal is asserted instead."""
import importlib.util
import json
import os
import sys

import numpy as np
import pytest
import torch

import _segloss_oracle as SO
import _segrefine_oracle as RO
from conftest import ROOT
from test_segloss_gpu import LABELS, TINY, make_labels, make_logits, on_device
from test_segrefine_cpu import BS, CS, GEOS, case_params, gpu_cases, logit_regime, make_guide, normal_case, refused

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RATIOS: dict = {}


def op_kwargs(p):
    return dict(iters=p["T"], radius=p["r"], dilation=p["d"], sigma_xy=p["sigma_xy"], sigma_i=p["sigma_i"], mix=p["lam"], weight=p["w"],
                inv_temperature=p["s"])


def judge(name, got, ref, bound, where):
    got, ref, bound = np.asarray(got, dtype=np.float64)[where], ref[where], bound[where]
    assert np.isfinite(got).all(), f"{name}: non-finite output"
    err = np.abs(got - ref)
    ratio = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print(f"{name}: error / bound = {ratio:.4g}")
    RATIOS[name] = max(RATIOS.get(name, 0.0), ratio)
    assert (err <= bound).all(), f"{name}: error / bound = {ratio:.3g}"


def against_oracle(name, z, guide, g, u, p, pred, conf):
    o = RO.refine(z, guide, g, u, **p)
    dec = o["decided"]
    assert (pred[dec] == o["pred"][dec]).all(), f"{name}: {(pred[dec] != o['pred'][dec]).sum()} decided pixels differ from the float64 arg-max"
    judge(name, conf, o["conf"], o["e_conf"], dec)
    return o


def one_case(g, u, B, C, i):
    from dinox import ops
    p, regime = case_params(i), logit_regime(i)
    S = g * u
    rng = np.random.default_rng([43, g, u, B, C, i])
    if regime == "normal":
        z, guide = normal_case(g, u, B, C, i)              # the arrays whose undecided share the CPU test caps
    else:
        z, guide = make_logits(rng, regime, B, g * g, C), make_guide(rng, B, S)
    y = make_labels(rng, LABELS[i % len(LABELS)], B, S, C)
    zt, gt, yt = on_device(z, i % 2), on_device(guide, (i // 2) % 2), torch.from_numpy(y).to(DEV)
    if refused(p, S):
        with pytest.raises(ValueError, match="no neighbour"):
            ops.seg_refine(zt, gt, u, yt, **op_kwargs(p))
        return
    pred, conf, counts = ops.seg_refine(zt, gt, u, yt, want_conf=True, **op_kwargs(p))
    pred_h, conf_h = pred.cpu().numpy(), conf.cpu().numpy()
    assert pred.dtype == torch.uint8 and conf.dtype == torch.float32 and counts.dtype == torch.int64 and tuple(counts.shape) == (3, C)
    assert ((conf_h >= 0) & (conf_h <= 1)).all() and (pred_h < C).all()
    assert np.array_equal(counts.cpu().numpy(), SO.counts(pred_h, y, C)), "counts differ from the recount of the returned map"
    o = against_oracle("conf", z, guide, g, u, p, pred_h, conf_h)
    if regime == "normal":
        assert 1.0 - o["decided"].mean() <= 0.05           # (the 1 % cap is held per geometry on the CPU; this only guards against a blank check)
    if i % 4 == 0:                                          # the same map without labels and without the confidence
        bare = ops.seg_refine(zt, gt, u, **op_kwargs(p))
        assert bare[1] is None and bare[2] is None and torch.equal(bare[0], pred)


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("g,u", GEOS)
def test_kernel_against_the_oracle(g, u, B, C):
    for i in gpu_cases(g, u, B, C):
        one_case(g, u, B, C, i)


def _inputs(g, u, B, C, seed, regime="normal"):
    rng = np.random.default_rng([47, g, u, B, C, seed])
    z, guide = make_logits(rng, regime, B, g * g, C), make_guide(rng, B, g * u)
    return z, guide, on_device(z, seed % 2), on_device(guide, 1 - seed % 2)


@pytest.mark.parametrize("g,u,B,C", [(1, 4, 3, 2), (3, 16, 3, 5), (14, 16, 1, 33), (2, 32, 1, 64), (5, 1, 3, 7)])
def test_zero_iterations_is_seg_predict_and_seg_calib(g, u, B, C):
    from dinox import ops
    for k, s in enumerate((1.0, 0.37, 2.5)):
        z, guide, zt, gt = _inputs(g, u, B, C, k, ("normal", "pm80", "dominant")[k])
        y = torch.from_numpy(make_labels(np.random.default_rng(k), "quarter ignored", B, g * u, C)).to(DEV)
        pred, conf, counts = ops.seg_refine(zt, gt, u, y, iters=0, radius=1, dilation=1, inv_temperature=s, want_conf=True)
        want_pred, want_counts = ops.seg_predict(zt, u, y)
        cal = ops.seg_calib(zt, u, inv_temperature=s, want_conf=True)
        assert torch.equal(pred, want_pred) and torch.equal(counts, want_counts) and torch.equal(pred, cal.pred)
        assert torch.equal(conf, cal.conf), "conf at T = 0 is not seg_calib's bit for bit"


@pytest.mark.parametrize("g,u,B,C", [(3, 16, 3, 5), (2, 3, 1, 33), (14, 16, 1, 2)])
def test_weight_zero_keeps_the_labels(g, u, B, C):
    """w = 0: V = U whatever the messages are, so the labels are those of T = 0."""
    from dinox import ops
    z, guide, zt, gt = _inputs(g, u, B, C, 3)
    for T, s in ((1, 1.0), (2, 0.37), (5, 2.5)):
        base, _, _ = ops.seg_refine(zt, gt, u, iters=0, radius=1, dilation=1, inv_temperature=s)
        got, _, _ = ops.seg_refine(zt, gt, u, iters=T, radius=1, dilation=1, weight=0.0, inv_temperature=s)
        assert torch.equal(got, base), f"T = {T}, s = {s}: {int((got != base).sum())} labels differ from T = 0"


def test_lambda_zero_ignores_the_guide_and_a_constant_guide_is_lambda_zero():
    from dinox import ops
    g, u, B, C = 3, 16, 2, 5
    z, guide, zt, gt = _inputs(g, u, B, C, 5)
    kw = dict(iters=3, radius=2, dilation=2, weight=4.0, want_conf=True)
    a = ops.seg_refine(zt, gt, u, mix=0.0, **kw)
    b = ops.seg_refine(zt, on_device(make_guide(np.random.default_rng(99), B, g * u) * 7, 0), u, mix=0.0, **kw)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), "lambda = 0: the guide changed the bits"
    flat = np.full((B, g * u, g * u), 0.731, dtype=np.float32)
    c = ops.seg_refine(zt, on_device(flat, 1), u, mix=0.8, **kw)
    p = dict(T=3, r=2, d=2, sigma_xy=3.0, sigma_i=0.5, lam=0.0, w=4.0, s=1.0)
    against_oracle("conf (constant guide vs lambda = 0)", z, flat, g, u, p, c[0].cpu().numpy(), c[1].cpu().numpy())
    against_oracle("conf (lambda = 0)", z, guide, g, u, p, a[0].cpu().numpy(), a[1].cpu().numpy())


@pytest.mark.parametrize("g,u,B,C,r,d", [(3, 16, 3, 5, 2, 2), (14, 16, 2, 33, 3, 1), (2, 32, 1, 64, 3, 8)])
def test_two_calls_give_the_same_bits(g, u, B, C, r, d):
    from dinox import ops
    z, guide, zt, gt = _inputs(g, u, B, C, 7)
    y = torch.from_numpy(make_labels(np.random.default_rng(7), "random", B, g * u, C)).to(DEV)
    outs = []
    for _ in range(2):
        outs.append([t.clone() for t in ops.seg_refine(zt, gt, u, y, iters=4, radius=r, dilation=d, want_conf=True)])
        torch.empty(1 << 20, device=DEV).normal_()          # other work between the calls
    assert all(torch.equal(a, b) for a, b in zip(*outs)) and bool(torch.isfinite(outs[0][1]).all())


def test_a_batch_is_its_images_one_by_one():
    """No halo leaks between images: B = 3 equals three calls of B = 1, bit for bit, with the widest window."""
    from dinox import ops
    g, u, B, C = 3, 16, 3, 5
    z, guide, zt, gt = _inputs(g, u, B, C, 9)
    kw = dict(iters=3, radius=3, dilation=8, sigma_xy=12.0, want_conf=True)
    whole = ops.seg_refine(zt, gt, u, **kw)
    for b in range(B):
        one = ops.seg_refine(zt[b:b + 1].contiguous(), gt[b:b + 1].contiguous(), u, **kw)
        assert torch.equal(one[0][0], whole[0][b]) and torch.equal(one[1][0], whole[1][b])


def test_non_finite_inputs_stay_inside_their_windows():
    """A NaN and a +inf logit and a NaN guide pixel: the call returns; wherever the float64 statement -- which spreads a non-finite value
    through the same windows -- stays finite, the outputs are held to it as everywhere else."""
    from dinox import ops
    g, u, B, C = 3, 16, 2, 5
    z, guide, _, _ = _inputs(g, u, B, C, 11)
    z[0, 4, 1], z[1, 0, 3] = np.nan, np.inf
    guide[0, 40, 7] = np.nan
    p = dict(T=2, r=2, d=2, sigma_xy=3.0, sigma_i=0.5, lam=0.8, w=4.0, s=1.0)
    pred, conf, _ = ops.seg_refine(on_device(z, 1), on_device(guide, 0), u, want_conf=True, **op_kwargs(p))
    torch.cuda.synchronize()
    o = RO.refine(z, guide, g, u, **p)
    clean = o["finite"]
    assert 0.05 < clean.mean() < 0.95 and (pred.cpu().numpy() < C).all()
    against_oracle("conf (clean pixels beside non-finite ones)", z, guide, g, u, p, pred.cpu().numpy(), conf.cpu().numpy())
    assert not np.isfinite(conf.cpu().numpy()[~clean]).all()


@pytest.mark.parametrize("g,u,d", [(1, 4, 3), (2, 3, 4), (5, 1, 3), (3, 4, 8)])
def test_a_dilation_that_empties_a_neighbourhood_is_refused(g, u, d):
    """r = 1 with S / 2 < d < S: r d < S, but the pixels with S - d <= x, y < d have every offset outside the image."""
    from dinox import ops
    z, guide, zt, gt = _inputs(g, u, 1, 3, 17)
    with pytest.raises(ValueError, match="no neighbour"):
        ops.seg_refine(zt, gt, u, radius=1, dilation=d)


@pytest.mark.parametrize("g,u,d", [(1, 4, 2), (2, 3, 3), (3, 4, 6), (5, 1, 2)])
def test_the_widest_dilation_allowed_keeps_every_pixel_a_neighbour(g, u, d):
    """r = 1 at 2 d = S (or S - 1): every pixel has exactly the neighbours on one side; conf is finite and held to the oracle."""
    from dinox import ops
    z, guide, zt, gt = _inputs(g, u, 2, 5, 19)
    p = dict(T=2, r=1, d=d, sigma_xy=3.0, sigma_i=0.5, lam=0.8, w=4.0, s=1.0)
    pred, conf, _ = ops.seg_refine(zt, gt, u, want_conf=True, **op_kwargs(p))
    conf_h = conf.cpu().numpy()
    assert np.isfinite(conf_h).all() and ((conf_h >= 0) & (conf_h <= 1)).all()
    o = against_oracle("conf (widest dilation)", z, guide, g, u, p, pred.cpu().numpy(), conf_h)
    assert o["finite"].all()


def test_refusals_on_the_device():
    from dinox import ops
    z, guide, zt, gt = _inputs(2, 3, 1, 2, 13)
    with pytest.raises(ValueError, match="no neighbour"):
        ops.seg_refine(zt, gt, 3, radius=3, dilation=2)
    with pytest.raises(ValueError, match="guide on"):
        ops.seg_refine(zt, gt.cpu(), 3)
    y = torch.zeros((1, 6, 6), dtype=torch.uint8, device=DEV)
    y[0, 2, 3] = 2                                          # >= C and not 255
    with pytest.raises(ValueError, match="1 label"):
        ops.seg_refine(zt, gt, 3, y, radius=1, dilation=1)


# ------------------------------------------------------------------------------------------ dinox.segment and the scripts end to end
def _script(name):
    if name in sys.modules:
        return sys.modules[name]
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "dino-x_amd", "scripts", name + ".py"))
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
    d = tmp_path_factory.mktemp("tiny_hub_refine")
    export_hub_checkpoint(m.to(DEV).eval(), d, config=dict(TINY, mlp_ratio=4.0, num_registers=4))
    return d


def test_segment_and_scripts_end_to_end(backbone_dir, tmp_path):
    from dinox import ops
    from dinox.segment import RefineConfig, load_segmenter, segment, segment_volume
    from zoo.encode import _batch
    fs, es, sv = _script("finetune_segmentation"), _script("evaluate_segmentation"), _script("segment_volume")
    out = tmp_path / "seg"
    res = fs.run(fs.parse_cli(["--backbone", str(backbone_dir), "--synthetic", "48", "--num-classes", "3", "--epochs", "2", "--batch-size", "12",
                               "--rank", "0", "--lr", "1e-2", "--warmup-epochs", "1", "--seed", "0", "--output", str(out)]))
    model = load_segmenter(backbone_dir, out, DEV)
    assert model.refine is None
    model.temperature = 1.7
    cfg = RefineConfig(iters=3, radius=1, dilation=2, sigma_i=0.3, weight=6.0)
    ds = res["val_dataset"]
    sx, sy, sz = ds.spacings[0].tolist()
    img = ds.images[0, 0].numpy()
    kw = dict(input_format="windowed_float")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        plain = segment(model, img, (sx, sy), sz, **kw)
        plain_c = segment(model, img, (sx, sy), sz, return_confidence=True, **kw)
        again = segment(model, img, (sx, sy), sz, refine=None, **kw)
        assert np.array_equal(plain, again) and np.array_equal(plain, plain_c[0])
        got, conf = segment(model, img, (sx, sy), sz, refine=cfg, return_confidence=True, **kw)
        only = segment(model, img, (sx, sy), sz, refine=cfg, **kw)
        with pytest.raises(ValueError, match="return_entropy"):
            segment(model, img, (sx, sy), sz, refine=cfg, return_entropy=True, **kw)
        # the same logits and guide through the op
        x = _batch([img], model.img_size, "windowed_float", 40.0, 400.0, DEV, "host")
        sp = torch.tensor([[sx, sy, sz]], dtype=torch.float32, device=DEV) if model.scale_aware else None
        with torch.no_grad():
            logits = model(x, spacing=sp)
        want, want_c, _ = ops.seg_refine(logits, x[:, 1].contiguous(), model.patch, inv_temperature=1.0 / 1.7, want_conf=True, **cfg.to_dict())
        assert np.array_equal(got, want[0].cpu().numpy()) and np.array_equal(conf, want_c[0].cpu().numpy()) and np.array_equal(only, got)
        assert got.dtype == np.uint8 and conf.dtype == np.float32 and got.shape == plain.shape
        # the volume: chunks of 2 over 5 slices equal one chunk; refine=None is today's output
        vol = np.random.default_rng(5).integers(31000, 35500, size=(5, 32, 32)).astype(np.uint16)
        vkw = dict(input_format="hu16_png")
        v_plain = segment_volume(model, vol, (1.0, 1.0, 2.0), batch_size=5, **vkw)
        assert np.array_equal(v_plain, segment_volume(model, vol, (1.0, 1.0, 2.0), batch_size=5, refine=None, **vkw))
        v1, c1 = segment_volume(model, vol, (1.0, 1.0, 2.0), batch_size=5, refine=cfg, return_confidence=True, **vkw)
        v2, c2 = segment_volume(model, vol, (1.0, 1.0, 2.0), batch_size=2, refine=cfg, return_confidence=True, **vkw)
        assert np.array_equal(v1, v2) and np.array_equal(c1, c2) and v1.shape == v_plain.shape and c1.dtype == np.float32
        assert np.array_equal(v1, segment_volume(model, vol, (1.0, 1.0, 2.0), batch_size=3, refine=cfg, **vkw))
    # scripts/evaluate_segmentation.py --refine: the "refine" block, and --write-refine
    base = ["--backbone", str(backbone_dir), "--segmenter", str(out), "--synthetic", "48", "--batch-size", "12", "--seed", "0"]
    r0 = es.run(es.build_parser().parse_args(base + ["--out", str(tmp_path / "e0.json")]))
    r1 = es.run(es.build_parser().parse_args(base + ["--refine", "--refine-iters", "2", "--refine-sigma-i", "0.3", "--write-refine",
                                                     "--out", str(tmp_path / "e1.json")]))
    assert "refine" not in r0
    blk = json.loads((tmp_path / "e1.json").read_text())["refine"]
    assert blk == r1["refine"] and blk["parameters"] == RefineConfig(iters=2, sigma_i=0.3).to_dict() and blk["temperature"] == 1.0
    assert blk["unrefined"]["dice"] == r0["per_class"]["dice"] and blk["unrefined"]["mean_dice"] == r0["mean"]["dice"]
    assert blk["unrefined"]["hd95_mm"] == r0["mean"]["hd95_mm"] and blk["unrefined"]["nsd"] == r0["mean"]["nsd"]
    assert blk["refined"]["dice"] == r1["per_class"]["dice"] and blk["refined"]["mean_dice"] == r1["mean"]["dice"]
    assert blk["refined"]["assd_mm"] == r1["mean"]["assd_mm"]
    print(f"evaluate --refine: mean Dice {blk['unrefined']['mean_dice']:.4f} -> {blk['refined']['mean_dice']:.4f}")
    # with a clean-up the pair is still raw against raw: the refined map before the clean-up, not the report's own (cleaned) scores
    r2 = es.run(es.build_parser().parse_args(base + ["--refine", "--refine-iters", "2", "--refine-sigma-i", "0.3", "--keep-largest",
                                                     "--out", str(tmp_path / "e2.json")]))
    assert r2["refine"]["unrefined"] == blk["unrefined"] and r2["refine"]["refined"] == blk["refined"]
    assert "before the clean-up" in r2["refine"]["clean_up"] and "none" in blk["clean_up"] and r2["postprocess"]["keep_largest"] is True
    stored = json.loads((out / "finetune_config.json").read_text())
    assert stored["refine"] == blk["parameters"] and stored["task"] == "segmentation"
    assert load_segmenter(backbone_dir, out, DEV).refine == RefineConfig(iters=2, sigma_i=0.3)
    # scripts/segment_volume.py --refine takes the stored parameters, flags replace single ones
    np.save(tmp_path / "vol.npy", vol)
    sv.run(sv.build_parser().parse_args(["--backbone", str(backbone_dir), "--segmenter", str(out), "--volume", str(tmp_path / "vol.npy"), "--spacing", "1",
                                         "1", "2", "--batch-size", "2", "--out", str(tmp_path / "lab.npy"), "--refine", "--refine-iters", "3",
                                         "--refine-radius", "1", "--refine-weight", "6", "--confidence-out", str(tmp_path / "conf.npy")]))
    m2 = load_segmenter(backbone_dir, out, DEV)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        w_l, w_c = segment_volume(m2, vol, (1.0, 1.0, 2.0), batch_size=5, refine=RefineConfig(iters=3, radius=1, sigma_i=0.3, weight=6.0),
                                  return_confidence=True, **vkw)
    assert np.array_equal(np.load(tmp_path / "lab.npy"), w_l) and np.array_equal(np.load(tmp_path / "conf.npy"), w_c)


def test_zz_report_error_to_bound_ratios():
    """Not a check of its own: prints the largest error / bound ratio every test above saw (each was asserted <= 1 there)."""
    for k in sorted(RATIOS):
        print(f"segrefine error/bound  {k:48s} {RATIOS[k]:.4f}")
