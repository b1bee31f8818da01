"""GPU tests of the surface-distance path: csrc/surfdist.hip (ops.surface_stats) against the float64 oracle (tests/_surface_oracle.py) within
its a-priori bounds with the counts exactly equal, determinism, independence of the batch cut, the bad-label refusal, a 1024 x 1024 map, and
scripts/evaluate_segmentation.py end to end.

Shapes (H, W): (1, 1) and the tails on both axes, W and H past one wave and past one 256-thread block.  A batch holds three images with
three spacings (s_y, s_x) = (1, 1), (0.7, 1.3), (2.5, 0.6).  Maps (``make_maps``): seeded blobs (an opening of smoothed noise, restated in
NumPy) plus, image 0, an object in the corner and a block of ignored pixels cutting through an object; image 1, a checkerboard patch in the
prediction (every pixel a border pixel); image 2, with C = 5 a class only in pred (2), one only in gt (3) and one in neither (4), with C = 2
class 1 only in pred.

Tolerances.  Counts can only be compared exactly where no exact distance sits on a tolerance, a condition on the INPUTS that the oracle
asserts (relative gap > 1e-5): {1.0, 2.0, 3.1} is paired with the spacing (0.7, 1.3) -- 49 a^2 + 169 b^2 is never 100, 400 or 961 -- and
also clear of (2.5, 0.6) (625 a^2 + 36 b^2 likewise); {1.5, 2.5} is paired with (1, 1) and (0.7, 1.3).  The mixed batch runs with both
sets; the within-tolerance counts of an image are compared in the call(s) whose set is paired with its spacing (every image in at least
one), n and the three floats of every image in every call."""
import importlib.util
import json
import os
import sys

import numpy as np
import pytest
import torch

import _surface_oracle as SO
from conftest import ROOT

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = ((1, 1), (8, 8), (33, 17), (64, 64), (40, 130), (300, 70))
SPACINGS = np.array([[1.0, 1.0], [0.7, 1.3], [2.5, 0.6]], dtype=np.float32)
TOLERANCES = (((1.0, 2.0, 3.1), (1, 2)), ((1.5, 2.5), (0, 1)))          # (set, images whose spacing it is paired with)
QUANTILES = ((95, 100), (1, 1), (1, 2))
OUTPUTS = ("sum", "max", "quantile")
RATIOS: dict = {}
_CASES: dict = {}


# ------------------------------------------------------------------------------------------ inputs
def _shifted(X, dy, dx):
    out = np.zeros_like(X)
    H, W = X.shape
    out[max(dy, 0):H + min(dy, 0), max(dx, 0):W + min(dx, 0)] = X[max(-dy, 0):H + min(-dy, 0), max(-dx, 0):W + min(-dx, 0)]
    return out


def opening(X):
    """binary_opening with the 4-connected cross, zeros outside the image."""
    er = X & _shifted(X, 1, 0) & _shifted(X, -1, 0) & _shifted(X, 0, 1) & _shifted(X, 0, -1)
    return er | _shifted(er, 1, 0) | _shifted(er, -1, 0) | _shifted(er, 0, 1) | _shifted(er, 0, -1)


def blobs(rng, H, W):
    n = rng.random((H + 4, W + 4))
    smooth = sum(n[i:i + H, j:j + W] for i in range(5) for j in range(5)) / 25.0
    return opening(smooth > 0.52)


def make_maps(H, W, C, seed):
    rng = np.random.default_rng([H, W, C, seed])
    pred, gt = np.zeros((3, H, W), np.uint8), np.zeros((3, H, W), np.uint8)
    for b in range(3):
        g = blobs(rng, H, W)
        gt[b][g] = 1
        pred[b][_shifted(g, 1, 2) | blobs(rng, H, W) & (rng.random((H, W)) < 0.5)] = 1
    gt[0, :min(3, H), :min(4, W)], pred[0, :min(4, H), :min(3, W)] = 1, 1                       # an object in the corner
    gt[0, H // 2:H // 2 + max(1, H // 4), W // 4:W // 4 + max(1, W // 2)] = 1                   # an object ...
    pred[0, H // 2:H // 2 + max(1, H // 4), W // 4:W // 4 + max(1, W // 2)] = 1
    gt[0, H // 3:H // 3 + max(1, H // 3), W // 2:W // 2 + max(1, W // 8)] = 255                 # ... and ignored pixels cutting through it
    ch, cw = min(H, 48), min(W, 48)
    yy, xx = np.mgrid[:ch, :cw]
    pred[1, (H - ch) // 2:(H - ch) // 2 + ch, (W - cw) // 2:(W - cw) // 2 + cw] = (yy + xx) % 2       # checkerboard
    if C >= 5:
        pred[2, H // 2:, :max(1, W // 3)] = 2                                                   # only in pred
        gt[2, :max(1, H // 3), W // 2:] = 3                                                     # only in gt; class 4 in neither
    else:
        gt[2] = 0                                                                               # class 1 only in pred
        pred[2, :max(1, H // 2), :max(1, W // 2)] = 1
    return pred, gt


def case(H, W, C):
    """(pred, gt, oracle distances) of a shape, built once and left unchanged."""
    key = (H, W, C)
    if key not in _CASES:
        pred, gt = make_maps(H, W, C, 0)
        _CASES[key] = (pred, gt, SO.Distances(pred, gt, SPACINGS, C))
    return _CASES[key]


def judge(name, got_counts, got_values, ref, within_images=None):
    counts, values, bound = ref
    gc, gv = got_counts.cpu().numpy(), got_values.double().cpu().numpy()
    assert gc.dtype == np.int64 and gc.shape == counts.shape and gv.shape == values.shape
    assert np.array_equal(gc[..., 0], counts[..., 0]), f"{name}: border pixel counts differ"
    imgs = range(counts.shape[0]) if within_images is None else within_images
    for b in imgs:
        assert np.array_equal(gc[b, ..., 1:], counts[b, ..., 1:]), f"{name}: within-tolerance counts of image {b} differ"
    assert np.isfinite(gv).all(), f"{name}: non-finite output"
    err = np.abs(gv - values)
    for i, out in enumerate(OUTPUTS):
        ratio = float((err[..., i] / np.maximum(bound[..., i], 1e-300)).max()) if (err[..., i] > 0).any() else 0.0
        print(f"{name} {out}: error / bound = {ratio:.4g}")
        RATIOS[out] = max(RATIOS.get(out, 0.0), ratio)
    assert (err <= bound).all(), f"{name}: error / bound = {(err / np.maximum(bound, 1e-300)).max():.3g}"


# ------------------------------------------------------------------------------------------ the kernel against the oracle
@pytest.mark.parametrize("C", (2, 5))
@pytest.mark.parametrize("H,W", SHAPES)
def test_kernel_against_the_oracle(H, W, C):
    from dinox import ops
    pred, gt, D = case(H, W, C)
    pt, gtt, sp = torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV), torch.from_numpy(SPACINGS).to(DEV)
    for tol, paired in TOLERANCES:
        gap = D.min_gap(tol)
        print(f"({H}, {W}) C={C} tolerances {tol}: smallest relative gap per image {gap}")
        assert all(gap[b] > 1e-5 for b in paired), f"an exact distance lies on a tolerance of {tol}: the inputs are wrong for this test"
        for q in QUANTILES:
            counts, values = ops.surface_stats(pt, gtt, sp, C, tolerances=tol, q=q)
            assert counts.is_cuda and values.is_cuda and values.dtype == torch.float32
            judge(f"({H}, {W}) C={C} tol={tol} q={q[0]}/{q[1]}", counts, values, D.stats(tol, q), paired)
            if q == (1, 1):
                assert torch.equal(values[..., 2], values[..., 1])              # the full quantile is the maximum, bit for bit


def test_empty_sides_give_zeros_and_the_counts_say_which():
    from dinox import ops
    pred, gt, D = case(33, 17, 5)
    counts, values = ops.surface_stats(torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV), torch.from_numpy(SPACINGS).to(DEV), 5,
                                       tolerances=(1.5, 2.5))
    c, v = counts.cpu(), values.cpu()
    assert c[2, 2, 0, 0] > 0 and c[2, 2, 1, 0] == 0 and c[2, 3, 0, 0] == 0 and c[2, 3, 1, 0] > 0 and not c[2, 4].any()
    for k in (2, 3, 4):
        assert not v[2, k].numpy().view(np.uint32).any() and not c[2, k, :, 1:].any()


# ------------------------------------------------------------------------------------------ determinism, chunking, bad labels
@pytest.mark.parametrize("H,W,C", ((33, 17, 5), (300, 70, 2)))
def test_two_calls_give_the_same_bits(H, W, C):
    from dinox import ops
    pred, gt, _ = case(H, W, C)
    args = (torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV), torch.from_numpy(SPACINGS).to(DEV), C)
    a = ops.surface_stats(*args, tolerances=(1.0, 2.0, 3.1))
    torch.empty(1 << 22, device=DEV).fill_(float("nan"))                       # whatever the next workspace holds must not matter
    b = ops.surface_stats(*args, tolerances=(1.0, 2.0, 3.1))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def test_forced_chunks_of_one_image_give_the_same_bits(monkeypatch):
    from dinox import ops
    pred, gt, _ = case(40, 130, 5)
    args = (torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV), torch.from_numpy(SPACINGS).to(DEV), 5)
    whole = ops.surface_stats(*args, tolerances=(1.5, 2.5))
    monkeypatch.setattr(ops, "SURFACE_WS_CAP", 1)                               # below one image's workspace: one image per call
    cut = ops.surface_stats(*args, tolerances=(1.5, 2.5))
    assert torch.equal(whole[0], cut[0]) and torch.equal(whole[1].view(torch.int32), cut[1].view(torch.int32))


def test_bad_labels_are_counted_and_refused():
    from dinox import ops
    pred, gt, _ = case(33, 17, 5)
    sp = torch.from_numpy(SPACINGS).to(DEV)
    p, g = torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV)
    bad = p.clone()
    bad[1, 5, 5], bad[2, 0, 0] = 5, 255                                         # in pred every value >= C is bad, 255 as well
    with pytest.raises(ValueError, match=r"2 value\(s\) of pred are >= C = 5, 0 label"):
        ops.surface_stats(bad, g, sp, 5)
    bad = g.clone()
    bad[0, 0, 0], bad[0, 1, 1], bad[2, 32, 16] = 255, 7, 64                     # 255 is ignore, not bad
    with pytest.raises(ValueError, match=r"0 value\(s\) of pred are >= C = 5, 2 label\(s\)"):
        ops.surface_stats(p, bad, sp, 5)
    for spacing in ([[1.0, 1.0], [0.0, 1.0], [1.0, 1.0]], [[1.0, float("nan")]] * 3, [[1.0, 1.0]] * 2):
        with pytest.raises(ValueError, match="spacing"):
            ops.surface_stats(p, g, spacing, 5)


def test_1024_square_with_one_small_object():
    from dinox import ops
    pred, gt = np.zeros((1, 1024, 1024), np.uint8), np.zeros((1, 1024, 1024), np.uint8)
    gt[0, 500:506, 600:607], pred[0, 503:509, 598:605] = 1, 1
    sp = np.array([[0.7, 1.3]], dtype=np.float32)
    D = SO.Distances(pred, gt, sp, 2)                                           # class 0: the image frame and a ring, 4k pixels a side
    tol = (1.0, 2.0, 3.1)
    assert D.min_gap(tol)[0] > 1e-5
    counts, values = ops.surface_stats(torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV), torch.from_numpy(sp), 2, tolerances=tol)
    assert int(counts[0, 0, 0, 0]) > 4000 and int(counts[0, 1, 1, 0]) == 22
    judge("(1024, 1024)", counts, values, D.stats(tol, (95, 100)))


# ------------------------------------------------------------------------------------------ scripts/evaluate_segmentation.py end to end
TINY = dict(img_size=32, patch=8, dim=32, depth=2, heads=2, scale_aware=True)      # the configuration tests/test_segloss_gpu.py trains


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
    d = tmp_path_factory.mktemp("tiny_hub_surface")
    export_hub_checkpoint(m.to(DEV).eval(), d, config=dict(TINY, mlp_ratio=4.0, num_registers=4))
    return d


def test_script_end_to_end(backbone_dir, tmp_path):
    from dinox import ops, segment as SG
    fs, es = _script("finetune_segmentation"), _script("evaluate_segmentation")
    seg = tmp_path / "seg"
    fs.run(fs.build_parser().parse_args(["--backbone", str(backbone_dir), "--synthetic", "48", "--num-classes", "3", "--epochs", "2", "--batch-size",
                                         "12", "--rank", "0", "--lr", "1e-2", "--warmup-epochs", "1", "--seed", "0", "--output", str(seg)]))
    out = tmp_path / "report" / "seg_eval.json"
    es.run(es.build_parser().parse_args(["--backbone", str(backbone_dir), "--segmenter", str(seg), "--synthetic", "48", "--batch-size", "5",
                                         "--out", str(out)]))
    rep = json.loads(out.read_text())
    assert set(rep) == {"images", "num_classes", "tolerances_mm", "quantile", "spacing", "pixel_accuracy", "per_class", "mean", "segmenter", "backbone"}
    assert set(rep["per_class"]) == {"dice", "iou", "hd95_mm", "assd_mm", "nsd", "surface_images", "overlap_images"}
    assert set(rep["mean"]) == {"dice", "iou", "hd95_mm", "assd_mm", "nsd", "classes"}
    assert rep["images"] == 12 and rep["num_classes"] == 3 and rep["tolerances_mm"] == [1.0, 2.0] and set(rep["per_class"]["nsd"]) == {"1", "2"}
    assert "(s_y, s_x)" in rep["spacing"]

    # the same validation set through load_segmenter and seg_predict, then the oracle on those label maps
    model = SG.load_segmenter(backbone_dir, seg, DEV)
    ds = es.EvalSynthetic(12, 32, 3, 0, first=36, augment=False)
    x = torch.stack([ds[i][0] for i in range(12)]).to(DEV)
    sp3 = torch.stack([ds[i][1] for i in range(12)]).to(DEV)
    masks = torch.stack([ds[i][2] for i in range(12)]).to(DEV)
    grid = torch.stack([ds[i][3] for i in range(12)])
    assert torch.equal(grid, ds.spacings[:, [1, 0]])                             # (s_y, s_x) of the set's own (x, y, z) spacings
    preds, cnt = [], 0
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        for i in range(0, 12, 5):                                                # the script's batches: the same launches, the same bits
            p, c = ops.seg_predict(model(x[i:i + 5], spacing=sp3[i:i + 5]), model.patch, masks[i:i + 5])
            preds.append(p)
            cnt = cnt + c
    pred = torch.cat(preds)
    assert rep["per_class"]["dice"] == SG.dice_per_class(cnt.cpu()).tolist() and rep["mean"]["dice"] == SG.mean_dice(cnt.cpu())
    assert rep["per_class"]["iou"] == SG.iou_per_class(cnt.cpu()).tolist()
    D = SO.Distances(pred.cpu().numpy(), masks.cpu().numpy(), grid.numpy(), 3)
    assert (D.min_gap((1.0, 2.0)) > 1e-5).all()
    counts, values, bound = D.stats((1.0, 2.0), (95, 100))
    ref = SO.metrics(counts, values, D.spacing, (32, 32))
    hi = SO.metrics(counts, values + bound, D.spacing, (32, 32))                 # the metrics are monotone in the three floats
    present = ~np.isnan(ref["hd95"])
    assert rep["per_class"]["surface_images"] == present.sum(0).tolist()
    for key, name in (("hd95", "hd95_mm"), ("assd", "assd_mm")):
        for c in range(3):
            got = rep["per_class"][name][c]
            if not present[:, c].any():
                assert got is None
                continue
            want, slack = np.nanmean(ref[key][:, c]), np.nanmean(hi[key][:, c] - ref[key][:, c])
            print(f"class {c} {name}: script {got}, oracle {want}, bound {slack:.3g}")
            assert abs(got - want) <= slack + 1e-15 * abs(want)
    for i, t in enumerate(("1", "2")):
        for c in range(3):
            if present[:, c].any():
                assert rep["per_class"]["nsd"][t][c] == pytest.approx(np.nanmean(ref["nsd"][:, c, i]), rel=1e-14, abs=1e-14)
    kept = [v for v in rep["per_class"]["hd95_mm"] if v is not None]
    assert rep["mean"]["hd95_mm"] == pytest.approx(sum(kept) / len(kept), rel=1e-14) and rep["mean"]["classes"] == len(kept)


def test_zz_report_error_to_bound_ratios():
    """Not a check of its own: prints the largest error / bound ratio every test above saw (each was asserted <= 1 there)."""
    for k in OUTPUTS:
        print(f"surface error/bound  {k:10s} {RATIOS.get(k, 0.0):.4f}")
