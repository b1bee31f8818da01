"""GPU tests of the 3-D surface-distance path: csrc/surfdist3d.hip (ops.surface_stats_3d) against the float64 oracle
(tests/_surface3d_oracle.py) within its a-priori bounds with the counts exactly equal, empty sides, determinism, independence of C, the
bad-label refusal, the anisotropic voxel, and scripts/segment_volume.py end to end.

Shapes (Z, H, W): one voxel, tails on every axis, W past a wave and past a strip of the y pass, Z past a wave, H past a 256-thread block,
and each axis at its limit of 1024 in turn.  Maps (``make_maps``): seeded 3-D blobs (an opening of smoothed noise, restated in NumPy) plus an
object in a corner, an object with a block of ignored voxels through it, a 3-D checkerboard patch in the prediction (every voxel a border
voxel) and an object whose prediction ends one slice early in z; with C = 5 a class only in pred (2), one only in gt (3) and one in neither
(4).  The volumes with a 1024 axis hold a few small objects at both ends of the long axis instead of blobs (small border lists for the
brute-force oracle, distances of a thousand voxels for the kernel).

Tolerances.  Counts can only be compared exactly where no exact distance sits on a tolerance, a condition on the INPUTS that the test
asserts (relative gap > 1e-5): {1.0, 2.0, 3.1} is paired with the voxel (2.5, 0.7, 1.3) -- 625 a^2 + 49 b^2 + 169 c^2 is never 100, 400 or
961 -- and {1.5, 2.5} with (1, 1, 1)."""
import importlib.util
import json
import os
import sys

import numpy as np
import pytest
import torch

import _surface3d_oracle as SO
from conftest import ROOT

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = ((1, 1, 1), (2, 3, 5), (5, 8, 8), (9, 33, 17), (3, 40, 130), (70, 9, 65), (4, 300, 6), (3, 5, 1024), (3, 1024, 5), (1024, 3, 5))
PAIRS = (((2.5, 0.7, 1.3), (1.0, 2.0, 3.1)), ((1.0, 1.0, 1.0), (1.5, 2.5)))           # (voxel (s_z, s_y, s_x), the tolerances paired with it)
QUANTILES = ((95, 100), (1, 1), (1, 2))
OUTPUTS = ("sum", "max", "quantile")
RATIOS: dict = {}
_CASES: dict = {}


# ------------------------------------------------------------------------------------------ inputs
def _shifted(X, d):
    out = np.zeros_like(X)
    src = tuple(slice(max(-k, 0), n + min(-k, 0)) for k, n in zip(d, X.shape))
    dst = tuple(slice(max(k, 0), n + min(k, 0)) for k, n in zip(d, X.shape))
    out[dst] = X[src]
    return out


CROSS = ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))


def opening(X):
    """binary_opening with the 6-connected cross, zeros outside the volume."""
    er = X.copy()
    for d in CROSS:
        er &= _shifted(X, d)
    out = er.copy()
    for d in CROSS:
        out |= _shifted(er, d)
    return out


def blobs(rng, Z, H, W):
    n = rng.random((Z + 2, H + 4, W + 4))
    smooth = sum(n[k:k + Z, i:i + H, j:j + W] for k in range(3) for i in range(5) for j in range(5)) / 75.0
    return opening(smooth > 0.535)


def make_maps(Z, H, W, C):
    rng = np.random.default_rng([Z, H, W, C])
    pred, gt = np.zeros((Z, H, W), np.uint8), np.zeros((Z, H, W), np.uint8)
    if max(Z, H, W) < 1024:
        g = blobs(rng, Z, H, W)
        gt[g] = 1
        pred[_shifted(g, (0, 1, 2)) | blobs(rng, Z, H, W) & (rng.random((Z, H, W)) < 0.5)] = 1
    else:                                                                                   # a small object at the far end of every axis
        gt[Z - min(Z, 3):, H - min(H, 3):, W - min(W, 4):] = 1
        pred[Z - min(Z, 2):, H - min(H, 3):, W - min(W, 6):] = 1
    gt[:min(2, Z), :min(3, H), :min(4, W)], pred[:min(2, Z), :min(4, H), :min(3, W)] = 1, 1     # an object in the corner
    box = (slice(None), slice(H // 2, H // 2 + max(1, H // 4)), slice(W // 4, W // 4 + max(1, min(W // 2, 40))))
    gt[box], pred[box] = 1, 1                                                               # an object through every slice ...
    gt[Z // 3:Z // 3 + max(1, Z // 3), H // 3:H // 3 + max(1, min(H // 3, 40)), W // 2:W // 2 + max(1, min(W // 8, 8))] = 255   # ... cut by ignored voxels
    cz, ch, cw = min(Z, 4), min(H, 6), min(W, 6)
    zz, yy, xx = np.mgrid[:cz, :ch, :cw]
    pred[(Z - cz) // 2:(Z - cz) // 2 + cz, (H - ch) // 2:(H - ch) // 2 + ch, (W - cw) // 2:(W - cw) // 2 + cw] = (zz + yy + xx) % 2      # checkerboard
    if Z >= 3:                                                                              # the prediction ends one slice early in z
        early = (slice(H - min(H, 5), H), slice(0, min(W, 5)))
        gt[(slice(0, Z - 1),) + early], pred[(slice(0, Z - 1),) + early], pred[(slice(Z - 2, Z - 1),) + early] = 1, 1, 0
    if C >= 5:
        pred[Z // 2:, H // 2:, :max(1, min(W // 3, 30))] = 2                                # only in pred
        gt[:, :max(1, min(H // 3, 30)), W // 2:W // 2 + max(1, min(W // 2, 30))] = 3        # only in gt; class 4 in neither
    return pred, gt


def case(Z, H, W, C):
    """(pred, gt, one oracle per voxel of PAIRS) of a shape, built once and left unchanged."""
    key = (Z, H, W, C)
    if key not in _CASES:
        pred, gt = make_maps(Z, H, W, C)
        _CASES[key] = (pred, gt, [SO.Distances(pred, gt, sp, C) for sp, _ in PAIRS])
    return _CASES[key]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def judge(name, got_counts, got_values, ref):
    counts, values, bound = ref
    gc, gv = got_counts.cpu().numpy(), got_values.double().cpu().numpy()
    assert gc.dtype == np.int64 and gc.shape == counts.shape and gv.shape == values.shape
    assert np.array_equal(gc[..., 0], counts[..., 0]), f"{name}: border voxel counts differ: {gc[..., 0].tolist()} vs {counts[..., 0].tolist()}"
    assert np.array_equal(gc[..., 1:], counts[..., 1:]), f"{name}: within-tolerance counts differ"
    assert np.isfinite(gv).all(), f"{name}: non-finite output"
    err = np.abs(gv - values)
    for i, out in enumerate(OUTPUTS):
        ratio = float((err[..., i] / np.maximum(bound[..., i], 1e-300)).max()) if (err[..., i] > 0).any() else 0.0
        print(f"{name} {out}: error / bound = {ratio:.4g}")
        RATIOS[out] = max(RATIOS.get(out, 0.0), ratio)
    assert (err <= bound).all(), f"{name}: error / bound = {(err / np.maximum(bound, 1e-300)).max():.3g}"


# ------------------------------------------------------------------------------------------ the kernel against the oracle
@pytest.mark.parametrize("C", (2, 5))
@pytest.mark.parametrize("Z,H,W", SHAPES)
def test_kernel_against_the_oracle(Z, H, W, C):
    from dinox import ops
    pred, gt, oracles = case(Z, H, W, C)
    pt, gtt = _dev(pred), _dev(gt)
    for (sp, tol), D in zip(PAIRS, oracles):
        gap = D.min_gap(tol)
        print(f"({Z}, {H}, {W}) C={C} voxel {sp} tolerances {tol}: smallest relative gap {gap}")
        assert gap > 1e-5, f"an exact distance lies on a tolerance of {tol}: the inputs are wrong for this test"
        for q in QUANTILES:
            counts, values = ops.surface_stats_3d(pt, gtt, sp, C, tolerances=tol, q=q)
            assert counts.is_cuda and values.is_cuda and values.dtype == torch.float32
            judge(f"({Z}, {H}, {W}) C={C} voxel={sp} q={q[0]}/{q[1]}", counts, values, D.stats(tol, q))
            if q == (1, 1):
                assert torch.equal(values.view(torch.int32)[..., 2], values.view(torch.int32)[..., 1])     # the full quantile is the maximum, bit for bit


def test_one_slice_is_all_border_and_not_the_2d_result():
    from dinox import ops
    pred, gt = np.zeros((1, 6, 7), np.uint8), np.zeros((1, 6, 7), np.uint8)
    gt[0, 1:5, 1:6], pred[0, 1:5, 2:7] = 1, 1
    c3, _ = ops.surface_stats_3d(_dev(pred), _dev(gt), (2.5, 0.7, 1.3), 2)
    c2, _ = ops.surface_stats(_dev(pred), _dev(gt), [[0.7, 1.3]], 2)
    assert c3[1, :, 0].tolist() == [20, 20] and c2[0, 1, :, 0].tolist() == [14, 14]


def test_empty_sides_give_zeros_and_the_counts_say_which():
    from dinox import ops
    pred, gt, _ = case(9, 33, 17, 5)
    counts, values = ops.surface_stats_3d(_dev(pred), _dev(gt), (1.0, 1.0, 1.0), 5, tolerances=(1.5, 2.5))
    c, v = counts.cpu(), values.cpu()
    assert c[2, 0, 0] > 0 and c[2, 1, 0] == 0 and c[3, 0, 0] == 0 and c[3, 1, 0] > 0 and not c[4].any()
    for k in (2, 3, 4):
        assert not v[k].numpy().view(np.uint32).any() and not c[k, :, 1:].any()


# ------------------------------------------------------------------------------------------ determinism, independence of C, bad labels
@pytest.mark.parametrize("Z,H,W,C", ((9, 33, 17, 5), (70, 9, 65, 2)))
def test_two_calls_give_the_same_bits(Z, H, W, C):
    from dinox import ops
    pred, gt, _ = case(Z, H, W, C)
    args = (_dev(pred), _dev(gt), (2.5, 0.7, 1.3), C)
    a = ops.surface_stats_3d(*args, tolerances=(1.0, 2.0, 3.1))
    torch.empty(1 << 22, device=DEV).fill_(float("nan"))                       # whatever the next workspace holds must not matter
    b = ops.surface_stats_3d(*args, tolerances=(1.0, 2.0, 3.1))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def test_a_class_does_not_depend_on_the_others():
    """The classes share one workspace, walked one at a time: class k under C = 5 equals class 1 of the maps reduced to k and background."""
    from dinox import ops
    pred, gt, _ = case(9, 33, 17, 5)
    whole = ops.surface_stats_3d(_dev(pred), _dev(gt), (2.5, 0.7, 1.3), 5, tolerances=(1.0, 2.0, 3.1))
    for k in (1, 2, 3, 4):
        p1 = (pred == k).astype(np.uint8)
        g1 = np.where(gt == 255, 255, gt == k).astype(np.uint8)
        alone = ops.surface_stats_3d(_dev(p1), _dev(g1), (2.5, 0.7, 1.3), 2, tolerances=(1.0, 2.0, 3.1))
        assert torch.equal(whole[0][k], alone[0][1]), k
        assert torch.equal(whole[1][k].view(torch.int32), alone[1][1].view(torch.int32)), k


def test_bad_labels_are_counted_and_refused():
    from dinox import ops
    pred, gt, _ = case(9, 33, 17, 5)
    p, g = _dev(pred), _dev(gt)
    bad = p.clone()
    bad[1, 5, 5], bad[8, 0, 0] = 5, 255                                         # in pred every value >= C is bad, 255 as well
    with pytest.raises(ValueError, match=r"surface_stats_3d: 2 value\(s\) of pred are >= C = 5, 0 label"):
        ops.surface_stats_3d(bad, g, (1.0, 1.0, 1.0), 5)
    bad = g.clone()
    bad[0, 0, 0], bad[0, 1, 1], bad[8, 32, 16] = 255, 7, 64                     # 255 is ignore, not bad
    with pytest.raises(ValueError, match=r"surface_stats_3d: 0 value\(s\) of pred are >= C = 5, 2 label\(s\)"):
        ops.surface_stats_3d(p, bad, (1.0, 1.0, 1.0), 5)


def test_the_slice_spacing_enters_the_distance():
    """An object whose prediction ends one slice early: HD95 is one slice spacing, whatever that is."""
    from dinox import ops
    pred, gt = np.zeros((8, 12, 12), np.uint8), np.zeros((8, 12, 12), np.uint8)
    gt[2:6, 3:9, 3:9], pred[2:5, 3:9, 3:9] = 1, 1
    got = {}
    for sz in (1.0, 5.0):
        D = SO.Distances(pred, gt, (sz, 1.0, 1.0), 2)
        counts, values, bound = D.stats((0.5,))
        c, v = ops.surface_stats_3d(_dev(pred), _dev(gt), (sz, 1.0, 1.0), 2, tolerances=(0.5,))
        judge(f"one slice early, s_z = {sz}", c, v, (counts, values, bound))
        assert max(values[1, 0, 2], values[1, 1, 2]) == sz                       # the oracle: the missing slice is s_z away
        got[sz] = float(torch.maximum(v[1, 0, 2], v[1, 1, 2]))
    assert got[1.0] == 1.0 and got[5.0] == 5.0


# ------------------------------------------------------------------------------------------ scripts/segment_volume.py end to end
TINY = dict(img_size=32, patch=8, dim=32, depth=2, heads=2, scale_aware=True)      # the configuration tests/test_cclabel3d_gpu.py builds
TODAY = {"cases", "connectivity", "overlap", "min_volume_mm3", "keep_largest", "per_class", "mean", "segmenter", "backbone"}
TODAY_PER_CLASS = {"dice", "dice_cases", "fp_per_case", "sensitivity", "precision", "f1", "n_gt", "n_gt_hit", "n_pred", "n_pred_hit"}
TODAY_MEAN = {"dice", "fp_per_case", "sensitivity", "precision", "f1"}


def _script():
    if "segment_volume" in sys.modules:
        return sys.modules["segment_volume"]
    spec = importlib.util.spec_from_file_location("segment_volume", os.path.join(ROOT, "dino-x_amd", "scripts", "segment_volume.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def seg_model():
    import zoo.arch as arch
    from dinox.segment import SegHead, SegModel
    torch.manual_seed(0)
    vit = arch.PatchViT(**TINY)
    with torch.no_grad():
        vit.scale_embed.mlp[2].weight.normal_(0, 0.05)
    head = SegHead(TINY["dim"], 3)
    with torch.no_grad():
        head.proj.weight.normal_(0, 1.0)
    return SegModel(vit, head).to(DEV).eval()


def test_script_end_to_end(seg_model, tmp_path, monkeypatch):
    sv = _script()
    monkeypatch.setattr(sv.SG, "load_segmenter", lambda backbone, segmenter, device: seg_model)       # the tiny model stands in for the files
    rng = np.random.default_rng(5)
    Z, H, W, S = 6, 40, 36, 32
    np.save(tmp_path / "vol.npy", rng.integers(31000, 35500, size=(Z, H, W)).astype(np.uint16))
    gt = np.zeros((Z, S, S), np.uint8)
    gt[1:5, 4:20, 6:22], gt[2:6, 18:30, 10:28], gt[0:2, 26:32, 0:5] = 1, 2, 255
    np.save(tmp_path / "gt.npy", gt)
    sp = ("1.1555555", "0.56", "2.5")                                            # the label grid's voxel: (2.5, 0.7, 1.3) up to rounding
    base = ["--backbone", "b", "--segmenter", "s", "--volume", str(tmp_path / "vol.npy"), "--labels", str(tmp_path / "gt.npy"), "--spacing", *sp,
            "--out", str(tmp_path / "out.npy"), "--no-amp"]
    plain = sv.run(sv.build_parser().parse_args(base + ["--report", str(tmp_path / "plain.json")]))
    assert set(plain) == TODAY and set(plain["per_class"]) == TODAY_PER_CLASS and set(plain["mean"]) == TODAY_MEAN
    sv.run(sv.build_parser().parse_args(base + ["--tolerance-mm", "1", "--tolerance-mm", "2", "--report", str(tmp_path / "rep.json")]))
    rep = json.loads((tmp_path / "rep.json").read_text())
    assert set(rep) == TODAY | {"tolerances_mm", "quantile", "spacing"}
    assert set(rep["per_class"]) == TODAY_PER_CLASS | {"hd95_mm", "assd_mm", "nsd", "surface_cases"}
    assert set(rep["mean"]) == TODAY_MEAN | {"hd95_mm", "assd_mm", "nsd"}
    assert rep["tolerances_mm"] == [1.0, 2.0] and rep["quantile"].startswith("95/100") and "(s_z, s_y, s_x)" in rep["spacing"]
    assert set(rep["per_class"]["nsd"]) == set(rep["mean"]["nsd"]) == {"1", "2"}
    for k in TODAY - {"per_class", "mean"}:
        assert rep[k] == plain[k], k
    for k in TODAY_PER_CLASS:
        assert rep["per_class"][k] == plain["per_class"][k], k

    out = np.load(tmp_path / "out.npy")
    assert out.shape == (Z, S, S) and len(np.unique(out)) > 1
    voxel = (float(sp[2]), float(sp[1]) * H / S, float(sp[0]) * W / S)
    D = SO.Distances(out, gt, voxel, 3)
    assert D.min_gap((1.0, 2.0)) > 1e-5
    counts, values, bound = D.stats((1.0, 2.0), (95, 100))
    ref = SO.metrics(counts, values, voxel, (Z, S, S))
    hi = SO.metrics(counts, values + bound, voxel, (Z, S, S))                    # the metrics are monotone in the three floats
    present = ~np.isnan(ref["hd95"][0])
    assert rep["per_class"]["surface_cases"] == present.astype(int).tolist() and present[1:].any()
    for key, name in (("hd95", "hd95_mm"), ("assd", "assd_mm")):
        for c in range(3):
            got = rep["per_class"][name][c]
            if not present[c]:
                assert got is None
                continue
            want, slack = ref[key][0, c], hi[key][0, c] - ref[key][0, c]
            print(f"class {c} {name}: script {got}, oracle {want}, bound {slack:.3g}")
            assert abs(got - want) <= slack + 1e-15 * abs(want)
        kept = [v for v in rep["per_class"][name][1:] if v is not None]
        assert rep["mean"][name] == pytest.approx(sum(kept) / len(kept), rel=1e-14)
    for i, t in enumerate(("1", "2")):
        for c in range(3):
            if present[c]:
                assert rep["per_class"]["nsd"][t][c] == pytest.approx(ref["nsd"][0, c, i], rel=1e-14, abs=1e-14)


def test_zz_report_error_to_bound_ratios():
    """Not a check of its own: prints the largest error / bound ratio every test above saw (each was asserted <= 1 there)."""
    for k in OUTPUTS:
        print(f"surface3d error/bound  {k:10s} {RATIOS.get(k, 0.0):.4f}")
