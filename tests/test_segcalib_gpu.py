"""GPU tests of the calibration path: csrc/segcalib.hip through ops.seg_calib against the float64 oracle (tests/_segcalib_oracle.py) within
its a-priori bounds, the histogram integer for integer against the kernel's own maps, pred bit for bit ops.seg_predict's, non-finite
logits, determinism, dinox.segment.fit_temperature on the device, and the scripts end to end.

Shapes: the segloss set (1, 4), (2, 3), (3, 16), (14, 16) plus (5, 1) -- one-pixel cells -- and (2, 32) -- the 48-wide cell, one row per
step; B = 1, 3; C = 2, 5, 33, 64.  Every (g, u, B, C) runs label x logit regimes (those of tests/test_segloss_gpu.py) with the bin count
(1, 10, 15, 64), the inverse temperature (1, 0.37, 2.5), the alignment of z (256 bytes / one float past) and that of the labels (4 bytes /
one byte past: at u % 8 == 0 the wide and the narrow label path) cycling through them: all fifteen regime pairs at the small geometries,
two per (B, C) at (14, 16), which together are all fifteen."""
import importlib.util
import json
import os
import sys

import numpy as np
import pytest
import torch

import _segcalib_oracle as CO
from conftest import ROOT
from test_segloss_gpu import LABELS, LOGITS, REGIMES, TINY, make_labels, make_logits, on_device

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GEOS = ((1, 4), (2, 3), (3, 16), (14, 16), (5, 1), (2, 32))
BS = (1, 3)
CS = (2, 5, 33, 64)
NBS = (1, 10, 15, 64)
SS = (1.0, 0.37, 2.5)
RATIOS: dict = {}
assert len(LABELS) * len(LOGITS) == len(REGIMES) == 15


def labels_on_device(y, offset):
    """y on the device, 4-byte aligned (offset 0) or one byte past that (offset 1)."""
    buf = torch.empty(y.size + 8, dtype=torch.uint8, device=DEV)
    start = (-buf.data_ptr()) % 4 + offset
    t = buf[start:start + y.size].view(y.shape)
    t.copy_(torch.from_numpy(y))
    assert t.data_ptr() % 4 == offset and t.is_contiguous()
    return t


def judge(name, got, ref, bound, where=None):
    got = np.asarray(got, dtype=np.float64).reshape(ref.shape)
    if where is not None:
        got, ref, bound = got[where], ref[where], bound[where]
    assert np.isfinite(got).all(), f"{name}: non-finite output"
    err = np.abs(got - ref)
    ratio = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print(f"{name}: error / bound = {ratio:.4g}")
    RATIOS[name] = max(RATIOS.get(name, 0.0), ratio)
    assert (err <= bound).all(), f"{name}: error / bound = {ratio:.3g}"


def check_histogram(res, y, C, NB):
    """hist and tail against the recomputation from the kernel's own pred and conf maps: integer for integer, no pixel exempt."""
    hist, tail = CO.histogram(res.pred.cpu().numpy(), res.conf.cpu().numpy(), y, C, NB)
    assert res.hist.dtype == torch.int64 and tuple(res.hist.shape) == (NB, 3) and tuple(res.tail.shape) == (3,)
    assert np.array_equal(res.hist.cpu().numpy(), hist), "histogram differs from the recomputation from the returned maps"
    assert np.array_equal(res.tail.cpu().numpy(), tail)
    return hist, tail


def one_case(g, u, B, C, i, lab_regime, log_regime):
    from dinox import ops
    NB, s, zoff, yoff = NBS[i % 4], SS[i % 3], (i // 2) % 2, (i // 3) % 2
    rng = np.random.default_rng([g, u, B, C, i])
    z = make_logits(rng, log_regime, B, g * g, C)
    y = make_labels(rng, lab_regime, B, g * u, C)
    zt, yt = on_device(z, zoff), labels_on_device(y, yoff)
    res = ops.seg_calib(zt, u, yt, inv_temperature=s, bins=NB, want_conf=True, want_entropy=True)
    assert torch.equal(res.pred, ops.seg_predict(zt, u)), "pred is not seg_predict's"
    if i % 5 == 0:                                          # the same maps without labels; the same sums without maps
        bare = ops.seg_calib(zt, u, inv_temperature=s, want_conf=True, want_entropy=True)
        assert bare.hist is None and all(torch.equal(a, b) for a, b in zip(bare[:3], res[:3]))
        lean = ops.seg_calib(zt, u, yt, inv_temperature=s, bins=NB, want_pred=False)
        assert lean.pred is None and lean.conf is None and torch.equal(lean.hist, res.hist) and torch.equal(lean.sums, res.sums)
    cal = CO.Calib(z, y, g, u)
    o = cal.at(s)
    conf, ent = res.conf.cpu().numpy(), res.entropy.cpu().numpy()
    share = 1.0 - cal.decided.mean()
    if log_regime == "normal":
        assert share <= 0.01, f"{share:.2%} of the pixels undecided in float64"
    assert (res.pred.cpu().numpy()[cal.decided] == cal.pred[cal.decided]).all()
    judge("conf", conf, o["conf"], o["e_conf"], cal.decided)
    judge("entropy", ent, o["entropy"], o["e_entropy"])
    assert ((conf >= 0) & (conf <= 1)).all() and ((ent >= 0) & (ent <= 1)).all()
    _, tail = check_histogram(res, y, C, NB)
    assert tail.tolist() == [o["nv"], 0, 0]
    sums = res.sums.cpu().numpy()
    if lab_regime == "all ignored":                         # exactly zero, bit for bit
        assert not sums.view(np.uint32).any() and not res.hist.any()
        return
    # none of the five sums depends on the arg-max (they are functions of p, l and y), so no pixel is exempt from their bounds
    for k, name in enumerate(CO.NAMES):
        judge(f"sum {name}", sums[k:k + 1], o["sums"][k:k + 1], o["e_sums"][k:k + 1])


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("g,u", GEOS)
def test_kernel_against_the_oracle(g, u, B, C):
    if g == 14:
        k = BS.index(B) * len(CS) + CS.index(C)
        todo = [(2 * k + j) % len(REGIMES) for j in range(2)]
    else:
        todo = range(len(REGIMES))
    for i in todo:
        one_case(g, u, B, C, i, *REGIMES[i])


def test_pm80_puts_confidences_on_bin_edges():
    """What the +-80 regime is for: confidences exactly 1.0 (the last bin by the clamp) and exactly 0.5 (an edge of NB = 10), every one
    in the bin the fp32 formula names."""
    from dinox import ops
    rng = np.random.default_rng(21)
    g, u, C, NB = 3, 16, 2, 10
    z = make_logits(rng, "pm80", 2, g * g, C)
    y = make_labels(rng, "random", 2, g * u, C)
    res = ops.seg_calib(on_device(z, 0), u, torch.from_numpy(y).to(DEV), bins=NB, want_conf=True)
    conf = res.conf.cpu().numpy()
    assert (conf == 1.0).any() and (conf == 0.5).any()
    hist, _ = check_histogram(res, y, C, NB)
    assert hist[NB - 1, 0] >= (conf == 1.0).sum() > 0 and hist[5, 0] >= (conf == 0.5).sum()


def test_non_finite_logits_enter_no_bin():
    """A NaN and a +inf in z: the call returns, the pixels they reach have a non-finite confidence, are counted in the tail and in no
    bin, and the histogram still equals the recomputation from the maps (every bin index stayed in range)."""
    from dinox import ops
    rng = np.random.default_rng(23)
    g, u, B, C, NB = 3, 16, 2, 5, 15
    z = make_logits(rng, "normal", B, g * g, C)
    z[0, 4, 1], z[1, 0, 3] = np.nan, np.inf
    y = make_labels(rng, "quarter ignored", B, g * u, C)
    res = ops.seg_calib(on_device(z, 1), u, torch.from_numpy(y).to(DEV), inv_temperature=0.37, bins=NB, want_conf=True, want_entropy=True)
    torch.cuda.synchronize()
    conf = res.conf.cpu().numpy()
    bad = ~np.isfinite(conf)
    assert bad.any() and not bad.all()
    hist, tail = check_histogram(res, y, C, NB)
    assert tail[2] == (bad & (y != 255)).sum() > 0 and hist[:, 0].sum() == tail[0] - tail[2]
    assert np.isfinite(res.sums.cpu().numpy()).all()
    assert torch.equal(res.pred, ops.seg_predict(on_device(z, 1), u))


@pytest.mark.parametrize("g,u,B,C", [(3, 16, 3, 5), (14, 16, 3, 33), (2, 32, 1, 64)])
def test_two_calls_give_the_same_bits(g, u, B, C):
    from dinox import ops
    rng = np.random.default_rng([9, g, C])
    zt = on_device(make_logits(rng, "normal", B, g * g, C), 1)
    yt = torch.from_numpy(make_labels(rng, "quarter ignored", B, g * u, C)).to(DEV)
    outs = []
    for _ in range(2):
        r = ops.seg_calib(zt, u, yt, inv_temperature=2.5, bins=15, want_conf=True, want_entropy=True)
        outs.append([t.clone() for t in r])
        torch.empty(1 << 20, device=DEV).normal_()          # other work between the calls
    assert all(torch.equal(a, b) for a, b in zip(*outs)) and all(bool(torch.isfinite(t).all()) for t in outs[0])


def test_bad_label():
    from dinox import ops
    rng = np.random.default_rng(7)
    z, y = make_logits(rng, "normal", 2, 9, 5), make_labels(rng, "quarter ignored", 2, 48, 5)
    zt = on_device(z, 0)
    y[1, 5, 7] = 5                                          # >= C and not 255: reported, never an address
    with pytest.raises(ValueError, match="1 label") as e:
        ops.seg_calib(zt, 16, torch.from_numpy(y).to(DEV))
    with pytest.raises(ValueError, match="1 label") as p:
        ops.seg_predict(zt, 16, torch.from_numpy(y).to(DEV))
    assert str(e.value).replace("seg_calib", "seg_predict") == str(p.value)


def test_fit_temperature_on_the_device():
    """Logits = 3 x a random field, labels drawn from the softmax of the unscaled upsampled field.  The fitted s must sit within
    tol + e_G / (s* H(s*)) of the oracle's root s* of G in log s: the step tolerance plus the first-order shift of the root under the
    kernel's error in G (e_G: the oracle's bound on the G total at s*)."""
    import _segloss_oracle as SO
    from dinox.segment import fit_temperature
    g, u, C, tol = 3, 16, 5, 1e-4
    rng = np.random.default_rng(31)
    host, dev = [], []
    for _ in range(2):
        f = rng.standard_normal((2, g * g, C)).astype(np.float32)
        l = SO.upsample(f, g, u)
        p = np.exp(l - l.max(-1, keepdims=True))
        p /= p.sum(-1, keepdims=True)
        y = (p.cumsum(-1) < rng.random(p.shape[:-1] + (1,))).sum(-1).clip(0, C - 1).astype(np.uint8)
        z = (3.0 * f).astype(np.float32)
        host.append(CO.Calib(z, y, g, u))
        dev.append((on_device(z, 0), torch.from_numpy(y).to(DEV)))
    fit = fit_temperature(dev, u, tol=tol)
    s_star = CO.root_of_g(host)
    e_G = sum(c.at(s_star)["e_sums"][2] for c in host)
    H = sum(c.newton(s_star)[2] for c in host)
    slack = tol + e_G / (s_star * H)
    gap = abs(np.log(1.0 / fit["temperature"]) - np.log(s_star))
    print(f"fitted temperature {fit['temperature']:.6f} (oracle root {1.0 / s_star:.6f}) in {fit['iterations']} steps; |log s - log s*| = {gap:.3e}, "
          f"allowed {slack:.3e}; NLL {fit['nll_before']:.6f} -> {fit['nll_after']:.6f}")
    assert fit["converged"] and gap <= slack
    assert fit["nll_after"] <= fit["nll_before"]


# ------------------------------------------------------------------------------------------ the scripts end to end
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
    d = tmp_path_factory.mktemp("tiny_hub_calib")
    export_hub_checkpoint(m.to(DEV).eval(), d, config=dict(TINY, mlp_ratio=4.0, num_registers=4))
    return d


def test_scripts_end_to_end(backbone_dir, tmp_path):
    from dinox.segment import load_segmenter, segment, segment_volume
    fs, es = _script("finetune_segmentation"), _script("evaluate_segmentation")
    out = tmp_path / "seg"
    argv = ["--backbone", str(backbone_dir), "--synthetic", "48", "--num-classes", "3", "--epochs", "4", "--batch-size", "12", "--rank", "0",
            "--lr", "1e-2", "--warmup-epochs", "1", "--seed", "0", "--output", str(out)]
    res = fs.run(fs.parse_cli(argv + ["--fit-temperature"]))
    cfg = json.loads((out / "finetune_config.json").read_text())
    T = cfg["temperature"]
    print(f"fitted temperature {T}: {res['temperature_fit']}")
    assert isinstance(T, float) and np.isfinite(T) and T > 0 and T == res["temperature_fit"]["temperature"]
    assert cfg["task"] == "segmentation" and cfg["best_epoch"] >= 1          # the rest of the file is what the run wrote before the fit
    model = load_segmenter(backbone_dir, out, DEV)
    assert model.temperature == T
    ds = res["val_dataset"]
    with torch.autocast("cuda", dtype=torch.bfloat16):
        for i in range(3):
            sx, sy, sz = ds.spacings[i].tolist()
            img = ds.images[i, 0].numpy()
            want = segment(model, img, (sx, sy), sz, input_format="windowed_float")
            got, conf, ent = segment(model, img, (sx, sy), sz, input_format="windowed_float", return_confidence=True, return_entropy=True)
            assert np.array_equal(got, want) and np.array_equal(want, res["val_pred"][i].numpy())
            assert conf.dtype == np.float32 and conf.shape == want.shape and (conf >= 1.0 / 3 - 1e-6).all() and (conf <= 1.0).all()
            assert ent.dtype == np.float32 and (ent >= 0).all() and (ent <= 1).all()
            got2, conf2 = segment(model, img, (sx, sy), sz, input_format="windowed_float", return_confidence=True, keep_largest=True)
            assert np.array_equal(conf2, conf)              # clean-up touches the labels only
        vol = np.random.default_rng(5).integers(31000, 35500, size=(4, 32, 32)).astype(np.uint16)      # what the script's default format reads
        kw = dict(input_format="hu16_png", batch_size=4)
        lv = segment_volume(model, vol, (1.0, 1.0, 2.0), **kw)
        lv2, cv = segment_volume(model, vol, (1.0, 1.0, 2.0), return_confidence=True, **kw)
        assert np.array_equal(lv, lv2) and cv.shape == lv.shape and cv.dtype == np.float32 and (cv <= 1.0).all() and (cv >= 1.0 / 3 - 1e-6).all()
        # the tiled path: the blend kernel's confidence; with T = 1 nothing is scaled and the labels are the bits of a run without the flag
        from dinox.segment import segment_volume_tiled
        tl = segment_volume_tiled(model, vol, (1.0, 1.0, 2.0), **kw)
        tl_t, tc = segment_volume_tiled(model, vol, (1.0, 1.0, 2.0), return_confidence=True, **kw)
        assert tl_t.shape == tc.shape == vol.shape and tc.dtype == np.float32 and (tc <= 1.0).all() and (tc >= 1.0 / 3 - 1e-6).all()
        assert (tl_t != tl).mean() <= 0.01                  # the blended logit over T: other labels only at fp32 near-ties
        model.temperature = 1.0
        tl_1, tc_1 = segment_volume_tiled(model, vol, (1.0, 1.0, 2.0), return_confidence=True, **kw)
        model.temperature = T
        assert np.array_equal(tl_1, tl) and not np.array_equal(tc_1, tc)
    # scripts/segment_volume.py writes the maps beside the labels
    sv = _script("segment_volume")
    np.save(tmp_path / "vol.npy", vol)
    sv_base = ["--backbone", str(backbone_dir), "--segmenter", str(out), "--volume", str(tmp_path / "vol.npy"), "--spacing", "1", "1", "2",
               "--batch-size", "4", "--out", str(tmp_path / "lab.npy")]
    sv.run(sv.build_parser().parse_args(sv_base + ["--confidence-out", str(tmp_path / "conf.npy"), "--entropy-out", str(tmp_path / "ent.npy")]))
    lab, cf, en = (np.load(tmp_path / f) for f in ("lab.npy", "conf.npy", "ent.npy"))
    assert lab.dtype == np.uint8 and cf.dtype == en.dtype == np.float32 and lab.shape == cf.shape == en.shape == (4, 32, 32)
    assert np.array_equal(lab, lv) and np.array_equal(cf, cv) and (en >= 0).all() and (en <= 1).all()
    sv.run(sv.build_parser().parse_args(sv_base + ["--tiled", "--confidence-out", str(tmp_path / "tconf.npy")]))
    assert np.array_equal(np.load(tmp_path / "lab.npy"), tl_t) and np.array_equal(np.load(tmp_path / "tconf.npy"), tc)
    base =["--backbone", str(backbone_dir), "--segmenter", str(out), "--synthetic", "48", "--batch-size", "12", "--seed", "0"]
    r0 = es.run(es.build_parser().parse_args(base + ["--out", str(tmp_path / "e0.json")]))
    r1 = es.run(es.build_parser().parse_args(base + ["--calibration", "--calibration-bins", "10", "--out", str(tmp_path / "e1.json")]))
    assert "calibration" not in r0
    cal = r1["calibration"]
    assert r1["per_class"]["dice"] == r0["per_class"]["dice"] and r1["per_class"]["iou"] == r0["per_class"]["iou"]      # the overlap scores do not move
    assert r1["mean"]["dice"] == r0["mean"]["dice"] and r1["mean"]["iou"] == r0["mean"]["iou"] and r1["pixel_accuracy"] == r0["pixel_accuracy"]
    assert json.loads((tmp_path / "e1.json").read_text())["calibration"]["pixels"] == cal["pixels"]
    assert cal["temperature"] == T and cal["num_bins"] == 10 and len(cal["bins"]) == 10
    assert cal["pixels"] == sum(b["count"] for b in cal["bins"] if b) > 0 and cal["nonfinite"] == 0
    assert 0 <= cal["ece"] <= cal["mce"] <= 1 and cal["nll"] > 0 and abs(cal["accuracy"] - r0["pixel_accuracy"]) < 1e-9
    r2 = es.run(es.build_parser().parse_args(base + ["--fit-temperature", "--temperature", "1.0", "--out", str(tmp_path / "e2.json")]))
    fit = r2["temperature_fit"]
    print(f"evaluate --fit-temperature: {fit}; ECE {r2['calibration']['ece']:.4f} -> {r2['calibration_fitted']['ece']:.4f}")
    assert r2["calibration"]["temperature"] == 1.0 and r2["calibration_fitted"]["temperature"] == fit["temperature"]
    assert r2["calibration_fitted"]["nll"] <= r2["calibration"]["nll"]
    assert json.loads((out / "finetune_config.json").read_text())["temperature"] == T      # not written without --write-temperature


def test_zz_report_error_to_bound_ratios():
    """Not a check of its own: prints the largest error / bound ratio every test above saw (each was asserted <= 1 there)."""
    for k in sorted(RATIOS):
        print(f"segcalib error/bound  {k:24s} {RATIOS[k]:.4f}")
