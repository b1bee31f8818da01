"""GPU tests of the connected-component path: csrc/cclabel.hip through ops.cc_label / cc_filter / lesion_counts, dinox.segment.postprocess
and segment(), and scripts/evaluate_segmentation.py, against the plain NumPy statement of the definitions in tests/_cc_oracle.py.
Everything is integers in a canonical form, so every comparison is exact (``torch.equal`` / ``==``): there is no tolerance in this file.

The kernel labels 32 x 32 tiles and flattens in chunks of 1024 pixels; the shapes straddle both (33 x 65, 63 x 129, 40 x 70) and the
structured maps (serpentine, comb, checkerboard, diagonal, the four-tile corner) are the cases in which the merge across tiles is all of
the work."""
import importlib.util
import json
import os
import sys

import numpy as np
import pytest
import torch

import _cc_oracle as CO
from conftest import ROOT

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def agree(got, want, what=""):
    """(comp, area, ncomp) of the kernel equal the oracle's, dtype and bits."""
    for g, w, dt, name in zip(got, want, (torch.int32, torch.int32, torch.int64), ("comp", "area", "ncomp")):
        assert g.is_cuda and g.dtype == dt and tuple(g.shape) == w.shape, (what, name)
        assert torch.equal(g.cpu(), torch.from_numpy(w)), f"{what}: {name} differs from the oracle"


def random_map(rng, B, H, W, C, p255=0.03):
    """Coarse blocks (components that span tiles) with single-pixel noise on top and some 255."""
    coarse = rng.integers(0, C, (B, -(-H // 5), -(-W // 5))).astype(np.uint8)
    m = np.repeat(np.repeat(coarse, 5, 1), 5, 2)[:, :H, :W].copy()
    noise = rng.random((B, H, W)) < 0.25
    m[noise] = rng.integers(0, C, int(noise.sum())).astype(np.uint8)
    m[rng.random((B, H, W)) < p255] = 255
    return m


def serpentine(H, W):
    """Corridors of class 1 on the even rows, joined at alternating ends: one component, its root (0, 0) at one end of a chain H W / 2 long."""
    m = np.zeros((1, H, W), np.uint8)
    m[0, ::2] = 1
    m[0, 1::4, W - 1] = 1
    m[0, 3::4, 0] = 1
    return m


# ------------------------------------------------------------------------------------------ labelling against the oracle
@pytest.mark.parametrize("conn", (4, 8))
@pytest.mark.parametrize("H,W", ((1, 1), (1, 37), (37, 1), (33, 65), (63, 129)))
def test_degenerate_and_partial_tiles(H, W, conn):
    from dinox import ops
    m = random_map(np.random.default_rng([H, W, conn]), 2, H, W, 3)
    agree(ops.cc_label(dev(m), 3, conn), CO.label_flood(m, 3, conn), f"({H}, {W}) conn {conn}")


@pytest.mark.parametrize("conn", (4, 8))
@pytest.mark.parametrize("C", (2, 3, 64))
def test_random_maps_with_ignored_pixels_a_mask_and_a_batch(C, conn):
    from dinox import ops
    rng = np.random.default_rng([C, conn])
    m = random_map(rng, 3, 40, 70, C)
    mask = np.where(rng.random(m.shape) < 0.05, 255, 0).astype(np.uint8)
    mask[0, 10:30, 33] = 255                                                    # a wall of masked pixels cutting components in two
    mask[mask == 0] = 7                                                         # any value but 255 leaves the pixel in
    for mk in (None, mask):
        got = ops.cc_label(dev(m), C, conn, None if mk is None else dev(mk))
        agree(got, CO.label_flood(m, C, conn, mk), f"C {C} conn {conn} mask {mk is not None}")
        for b in range(3):                                                      # an image's result does not depend on its batch
            one = ops.cc_label(dev(m[b:b + 1]), C, conn, None if mk is None else dev(mk[b:b + 1]))
            assert all(torch.equal(o[0], g[b]) for o, g in zip(one, got)), f"image {b}"


@pytest.mark.parametrize("conn", (4, 8))
@pytest.mark.parametrize("S", (64, 1024))
def test_serpentine(S, conn):
    from dinox import ops
    m = serpentine(S, S)
    want = CO.label_runs(m, 2, conn)
    assert want[2].tolist() == [[S // 2, 1]] and want[1][0, 0, 0] == S // 2 * S + S // 2 and (want[0][0][m[0] == 1] == 0).all()
    agree(ops.cc_label(dev(m), 2, conn), want, f"serpentine {S} conn {conn}")


@pytest.mark.parametrize("conn", (4, 8))
def test_rectangular_serpentine_and_comb(conn):
    from dinox import ops
    m = serpentine(70, 100)
    comb = np.zeros((1, 70, 100), np.uint8)
    comb[0, :, ::2] = 1                                                         # teeth ...
    comb[0, 69, :] = 1                                                          # ... that join only in the last row: the root travels back up every tooth
    both = np.concatenate([m, comb])
    want = CO.label_flood(both, 2, conn)
    assert want[2][1, 1] == 1 and (want[0][1][comb[0] == 1] == 0).all()
    agree(ops.cc_label(dev(both), 2, conn), want, f"serpentine and comb, conn {conn}")


def test_checkerboard_of_two_classes():
    from dinox import ops
    H, W = 66, 70
    yy, xx = np.mgrid[:H, :W]
    m = ((yy + xx) % 2).astype(np.uint8)[None]
    comp, area, ncomp = ops.cc_label(dev(m), 2, 4)
    assert ncomp.tolist() == [[H * W // 2, H * W // 2]]
    assert torch.equal(comp[0].cpu(), torch.arange(H * W, dtype=torch.int32).view(H, W)) and bool((area == 1).all())
    got = ops.cc_label(dev(m), 2, 8)
    assert got[2].tolist() == [[1, 1]] and got[1][0, 0, 0] == H * W // 2 and got[1][0, 0, 1] == H * W // 2
    agree(got, CO.label_flood(m, 2, 8), "checkerboard conn 8")


def test_diagonal_line_across_tile_corners():
    from dinox import ops
    H = 97
    m = np.eye(H, dtype=np.uint8)[None]                                         # passes (31, 31) -> (32, 32) and (63, 63) -> (64, 64)
    anti = np.ascontiguousarray(m[:, :, ::-1])                                  # and (31, 65) -> (32, 64): the north-east unions
    for mm in (m, anti):
        got = ops.cc_label(dev(mm), 2, 8)
        assert got[2][0, 1] == 1 and int(got[1].max()) >= H
        agree(got, CO.label_flood(mm, 2, 8), "diagonal conn 8")
        got = ops.cc_label(dev(mm), 2, 4)
        assert got[2][0, 1] == H
        agree(got, CO.label_flood(mm, 2, 4), "diagonal conn 4")


def test_component_that_touches_four_tiles_at_their_corner_only():
    from dinox import ops
    m = np.zeros((1, 64, 64), np.uint8)
    m[0, 31, 31] = m[0, 32, 32] = 1
    m[0, 31, 32] = m[0, 32, 31] = 2
    got = ops.cc_label(dev(m), 3, 8)
    assert got[2].tolist() == [[1, 1, 1]] and got[0][0, 32, 32] == 31 * 64 + 31 and got[0][0, 32, 31] == 31 * 64 + 32
    agree(got, CO.label_flood(m, 3, 8), "four tiles conn 8")
    got = ops.cc_label(dev(m), 3, 4)
    assert got[2].tolist() == [[1, 2, 2]]
    agree(got, CO.label_flood(m, 3, 4), "four tiles conn 4")
    full = np.full((1, 64, 64), 1, np.uint8)                                    # and one component that fills all four
    got = ops.cc_label(dev(full), 2, 4)
    assert got[2].tolist() == [[0, 1]] and got[1][0, 0, 0] == 4096 and not bool(got[0].any())


def test_values_outside_the_classes():
    from dinox import ops
    m = random_map(np.random.default_rng(9), 2, 33, 40, 3, p255=0.0)
    bad = m.copy()
    bad[0, 5, 5], bad[1, 32, 39], bad[1, 0, 0] = 3, 200, 255                    # 255 is no component, not an error
    with pytest.raises(ValueError, match=r"cc_label: 2 value\(s\) of labels are >= C = 3"):
        ops.cc_label(dev(bad), 3)
    mask = np.zeros_like(m)
    mask[0, 5, 5] = mask[1, 32, 39] = 255                                       # under the mask they are not counted
    agree(ops.cc_label(dev(bad), 3, 8, dev(mask)), CO.label_flood(bad, 3, 8, mask), "bad values under the mask")
    with pytest.raises(ValueError, match=r"lesion_counts: 2 value\(s\) of labels"):
        ops.lesion_counts(dev(m), dev(bad), 3)
    with pytest.raises(ValueError, match=r"lesion_counts: 2 value\(s\) of pred"):
        ops.lesion_counts(dev(bad), dev(m), 3)
    with pytest.raises(ValueError, match=r"cc_filter: 2 value\(s\) of labels"):
        ops.cc_filter(dev(bad), 3)
    with pytest.raises(ValueError, match=r"cc_filter: 2 label\(s\) are >= C = 3"):
        ops.cc_filter(dev(m), 3, targets=dev(bad))


def test_two_calls_give_the_same_bits_and_the_cut_does_not_matter(monkeypatch):
    from dinox import ops
    rng = np.random.default_rng(21)
    m, g = random_map(rng, 3, 63, 129, 3), random_map(rng, 3, 63, 129, 3)
    a = ops.cc_label(dev(m), 3, 8) + (ops.cc_filter(dev(m), 3, min_px=5, keep_largest=True), ops.lesion_counts(dev(m), dev(g), 3, min_px=[1, 4, 9]))
    torch.empty(1 << 22, dtype=torch.int32, device=DEV).fill_(-7)               # whatever the next workspace holds must not matter
    b = ops.cc_label(dev(m), 3, 8) + (ops.cc_filter(dev(m), 3, min_px=5, keep_largest=True), ops.lesion_counts(dev(m), dev(g), 3, min_px=[1, 4, 9]))
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    monkeypatch.setattr(ops, "CC_WS_CAP", 1)                                    # below one image's workspace: one image per call
    c = ops.cc_label(dev(m), 3, 8) + (ops.cc_filter(dev(m), 3, min_px=5, keep_largest=True), ops.lesion_counts(dev(m), dev(g), 3, min_px=[1, 4, 9]))
    assert all(torch.equal(x, y) for x, y in zip(a, c))
    out, counts = ops.cc_filter(dev(m), 3, min_px=5, targets=dev(g))
    whole = CO.overlap_counts(CO.cc_filter(m, 3, min_px=[5] * 3), np.where(g >= 3, 255, g), 3)[0]
    assert counts.tolist() == whole.tolist()


# ------------------------------------------------------------------------------------------ the filter
def test_keep_largest_with_an_exact_tie():
    from dinox import ops
    m = np.zeros((2, 40, 70), np.uint8)
    m[0, 30:33, 60:64] = 1                                                      # 12 pixels, later in raster order, across a tile edge
    m[0, 2:6, 3:6] = 1                                                          # 12 pixels, first: wins the tie
    m[0, 10:12, 10:15] = 1                                                      # 10 pixels
    m[0, 20:22, 20:22] = 2                                                      # class 2 has its own largest
    m[1, 5, 5] = 1                                                              # image 1: a single pixel is the largest
    out = ops.cc_filter(dev(m), 3, keep_largest=True)
    want = np.zeros_like(m)
    want[0, 2:6, 3:6], want[0, 20:22, 20:22], want[1, 5, 5] = 1, 2, 1
    assert out.dtype == torch.uint8 and torch.equal(out.cpu(), torch.from_numpy(want))
    assert np.array_equal(CO.cc_filter(m, 3, keep_largest=True), want)


@pytest.mark.parametrize("conn", (4, 8))
def test_filter_options_against_the_oracle(conn):
    from dinox import ops
    rng = np.random.default_rng([3, conn])
    m = random_map(rng, 3, 40, 70, 4)
    y = random_map(rng, 3, 40, 70, 4, p255=0.1)
    mp = [1, 6, 40]
    for kw in (dict(min_px=mp), dict(keep_largest=True), dict(min_px=mp, keep_largest=True), dict(min_px=mp, first_class=2),
               dict(min_px=4, first_class=0), dict()):
        out, counts = ops.cc_filter(dev(m), 4, connectivity=conn, targets=dev(y), **kw)
        okw = dict(kw, min_px=[kw["min_px"]] * 3) if isinstance(kw.get("min_px"), int) else kw
        want = CO.cc_filter(m, 4, connectivity=conn, **okw)
        assert torch.equal(out.cpu(), torch.from_numpy(want)), kw
        assert torch.equal(out, ops.cc_filter(dev(m), 4, connectivity=conn, **kw))
        o = out.long()
        yl, valid = dev(y).long(), dev(y) != 255                               # seg_predict's counts in torch integer ops on out
        ref = torch.stack([torch.stack([((o == c) & (yl == c) & valid).sum(), ((o == c) & valid).sum(), ((yl == c) & valid).sum()]) for c in range(4)], 1)
        assert counts.dtype == torch.int64 and counts.shape == (3, 4) and torch.equal(counts, ref), kw
        assert counts.tolist() == CO.overlap_counts(want, y, 4)[0].tolist()
        first = okw.get("first_class", 1)
        assert torch.equal(out.cpu()[torch.from_numpy((m < first))], torch.from_numpy(m[m < first]))          # the classes below first_class: untouched
    masked = ops.cc_filter(dev(m), 4, connectivity=conn, min_px=mp, mask=dev(y))
    assert torch.equal(masked.cpu(), torch.from_numpy(CO.cc_filter(m, 4, min_px=mp, connectivity=conn, mask=y)))


# ------------------------------------------------------------------------------------------ lesion-wise counts
def _pair():
    return np.zeros((1, 40, 70), np.uint8), np.zeros((1, 40, 70), np.uint8)


def _counts(pred, gt, C=2, **kw):
    from dinox import ops
    got = ops.lesion_counts(dev(pred), dev(gt), C, **kw)
    assert got.dtype == torch.int64 and got.shape == (pred.shape[0], C, 4)
    assert got.tolist() == CO.lesion_counts(pred, gt, C, **kw).tolist()
    return got[0, 1].tolist()


def test_missed_split_and_merged_lesions():
    pred, gt = _pair()
    gt[0, 5:9, 5:9] = 1                                                         # found
    gt[0, 20:24, 50:54] = 1                                                     # missed
    pred[0, 6:10, 6:10] = 1
    pred[0, 30:33, 10:13] = 1                                                   # invented
    assert _counts(pred, gt) == [2, 1, 2, 1]
    pred, gt = _pair()
    gt[0, 10:14, 20:40] = 1                                                     # one lesion (across a tile edge) ...
    pred[0, 10:14, 20:28] = pred[0, 10:14, 32:40] = 1                           # ... found as two
    assert _counts(pred, gt) == [1, 1, 2, 2]
    assert _counts(gt, pred) == [2, 2, 1, 1]                                    # merged: two lesions under one prediction


def test_overlap_threshold_just_under_and_exactly_at():
    pred, gt = _pair()
    gt[0, 4:8, 4:9] = 1                                                         # 20 pixels
    pred[0, 4:8, 7:12] = 1                                                      # 20 pixels, 8 shared: 8 / 20 = 2 / 5
    assert _counts(pred, gt, overlap=(2, 5)) == [1, 1, 1, 1]                    # exactly at the threshold
    assert _counts(pred, gt, overlap=(401, 1000)) == [1, 0, 1, 0]               # just under it
    assert _counts(pred, gt, overlap=(0, 1)) == [1, 1, 1, 1]
    pred[0, 4, 12] = 1                                                          # 21 pixels on one side only: 8 / 21 < 2 / 5
    assert _counts(pred, gt, overlap=(2, 5)) == [1, 1, 1, 0]
    assert _counts(pred, gt, overlap=(1, 1)) == [1, 0, 1, 0]
    assert _counts(gt, gt, overlap=(1, 1)) == [1, 1, 1, 1]


def test_min_px_on_one_side_and_ignored_pixels_cutting_a_prediction():
    pred, gt = _pair()
    gt[0, 4:6, 4:6] = 1                                                         # 4 pixels
    pred[0, 4:7, 4:7] = 1                                                       # 9 pixels over it
    assert _counts(pred, gt, min_px=[5]) == [0, 0, 1, 1]                        # no lesion on the gt side; its pixels still match the prediction
    assert _counts(pred, gt, min_px=[10]) == [0, 0, 0, 0] and _counts(pred, gt, min_px=[4]) == [1, 1, 1, 1]
    pred, gt = _pair()
    gt[0, 10:13, 10:30] = 1
    pred[0, 10:13, 10:30] = 1
    gt[0, :, 20] = 255                                                          # an ignored column cuts both in two
    assert _counts(pred, gt) == [2, 2, 2, 2]
    gt[0, 10:13, 21:30] = 0                                                     # and the right half of the prediction is now a false positive
    assert _counts(pred, gt) == [1, 1, 2, 1]


@pytest.mark.parametrize("conn", (4, 8))
def test_lesion_counts_on_random_maps(conn):
    from dinox import ops
    rng = np.random.default_rng([11, conn])
    gt = random_map(rng, 3, 63, 129, 3, p255=0.05)
    pred = np.where(rng.random(gt.shape) < 0.7, np.where(gt == 255, 0, gt), random_map(rng, 3, 63, 129, 3, p255=0.01)).astype(np.uint8)
    for kw in (dict(), dict(overlap=(1, 2)), dict(overlap=(1, 2), min_px=[1, 3, 12])):
        got = ops.lesion_counts(dev(pred), dev(gt), 3, connectivity=conn, **kw)
        want = CO.lesion_counts(pred, gt, 3, connectivity=conn, **kw)
        assert got.tolist() == want.tolist(), kw
        assert want[..., 0].sum() > want[..., 1].sum() > 0 and want[..., 2].sum() > want[..., 3].sum() > 0      # hits and misses on both sides


# ------------------------------------------------------------------------------------------ dinox.segment and the script on the tiny model
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
def trained(tmp_path_factory):
    """(backbone directory, segmenter directory) of a run on --synthetic 48, the set tests/test_surface_gpu.py evaluates, with 16 epochs: after
    its two the head still predicts background everywhere, and a clean-up with nothing to remove would show nothing."""
    import zoo.arch as arch
    from zoo.hub import export_hub_checkpoint
    torch.manual_seed(0)
    m = arch.PatchViT(**TINY)
    with torch.no_grad():
        m.scale_embed.mlp[2].weight.normal_(0, 0.05)
    d = tmp_path_factory.mktemp("tiny_hub_cc")
    export_hub_checkpoint(m.to(DEV).eval(), d, config=dict(TINY, mlp_ratio=4.0, num_registers=4))
    fs = _script("finetune_segmentation")
    seg = tmp_path_factory.mktemp("seg_cc")
    fs.run(fs.build_parser().parse_args(["--backbone", str(d), "--synthetic", "48", "--num-classes", "3", "--epochs", "16", "--batch-size", "12", "--rank",
                                         "0", "--lr", "1e-2", "--warmup-epochs", "1", "--seed", "0", "--output", str(seg)]))
    return d, seg


def test_postprocess_and_segment(trained):
    from dinox import segment as SG
    rng = np.random.default_rng(4)
    m = random_map(rng, 3, 40, 70, 3, p255=0.0)
    sp = np.array([[1.0, 1.0], [0.5, 0.7], [2.0, 1.5]], np.float32)
    for kw in (dict(min_area_mm2=6.0), dict(keep_largest=True), dict(keep_largest=True, min_area_mm2=30.0, connectivity=4), dict()):
        got = SG.postprocess(dev(m), 3, sp, **kw)
        want = CO.cc_filter(m, 3, min_px=CO.min_px(kw.get("min_area_mm2", 0.0), sp), keep_largest=kw.get("keep_largest", False),
                            connectivity=kw.get("connectivity", 8))
        assert torch.equal(got.cpu(), torch.from_numpy(want)), kw
    assert torch.equal(SG.postprocess(dev(m), 3).cpu(), torch.from_numpy(m))                  # nothing asked for: nothing changes
    model = SG.load_segmenter(*trained, DEV)
    ds = _script("evaluate_segmentation").EvalSynthetic(12, 32, 3, 0, first=36, augment=False)
    changed = 0
    with torch.autocast("cuda", dtype=torch.bfloat16):
        for i in range(12):
            sx, sy, sz = ds.spacings[i].tolist()
            plain = SG.segment(model, ds.images[i, 0].numpy(), (sx, sy), sz, input_format="windowed_float")
            same = SG.segment(model, ds.images[i, 0].numpy(), (sx, sy), sz, input_format="windowed_float", keep_largest=False, min_area_mm2=0.0)
            assert np.array_equal(plain, same)
            got = SG.segment(model, ds.images[i, 0].numpy(), (sx, sy), sz, input_format="windowed_float", keep_largest=True, min_area_mm2=150.0)
            grid = np.array([[sy, sx]], np.float64)                                           # a 32 x 32 image on the 32 x 32 grid: its own spacing
            want = CO.cc_filter(plain[None], 3, min_px=CO.min_px(150.0, grid), keep_largest=True)[0]
            assert got.dtype == np.uint8 and np.array_equal(got, want), f"image {i}"
            changed += int((got != plain).sum())
    print(f"segment(keep_largest=True, min_area_mm2=150): {changed} pixel(s) changed over 12 images")
    assert changed > 0


OLD_KEYS = {"images", "num_classes", "tolerances_mm", "quantile", "spacing", "pixel_accuracy", "per_class", "mean", "segmenter", "backbone"}


def test_script_end_to_end(trained, tmp_path):
    from dinox import ops, segment as SG
    backbone_dir, seg = trained
    es = _script("evaluate_segmentation")
    base = ["--backbone", str(backbone_dir), "--segmenter", str(seg), "--synthetic", "48", "--batch-size", "5"]
    out = tmp_path / "report" / "seg_eval.json"
    es.run(es.build_parser().parse_args(base + ["--out", str(out), "--lesion-metrics", "--keep-largest", "--min-component-mm2", "60.0", "--lesion-overlap",
                                                "0.2504", "--connectivity", "4"]))
    rep = json.loads(out.read_text())
    assert set(rep) == OLD_KEYS | {"lesion", "postprocess"}
    assert rep["postprocess"] == {"keep_largest": True, "min_area_mm2": 60.0, "connectivity": 4}
    les = rep["lesion"]
    assert (les["connectivity"], les["overlap"], les["min_area_mm2"], les["images"]) == (4, "250/1000", 60.0, 12)

    # the same label maps through load_segmenter and seg_predict, then the oracle's filter, counts and metrics
    model = SG.load_segmenter(backbone_dir, seg, DEV)
    ds = es.EvalSynthetic(12, 32, 3, 0, first=36, augment=False)
    x = torch.stack([ds[i][0] for i in range(12)]).to(DEV)
    sp3 = torch.stack([ds[i][1] for i in range(12)]).to(DEV)
    masks = torch.stack([ds[i][2] for i in range(12)])
    grid = torch.stack([ds[i][3] for i in range(12)]).numpy()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        pred = torch.cat([ops.seg_predict(model(x[i:i + 5], spacing=sp3[i:i + 5]), model.patch) for i in range(0, 12, 5)]).cpu().numpy()
    mp = CO.min_px(60.0, grid)
    clean = CO.cc_filter(pred, 3, min_px=mp, keep_largest=True, connectivity=4)
    print(f"min_px per image {mp}; the filter changed {(clean != pred).sum()} of {pred.size} pixels")
    assert (clean != pred).any() and clean.any()                               # the run has something to remove and something to keep
    want = CO.lesion_metrics(CO.lesion_counts(clean, masks.numpy(), 3, connectivity=4, overlap=(250, 1000), min_px=mp))
    for k in ("n_gt", "n_gt_hit", "n_pred", "n_pred_hit"):
        assert les["per_class"][k] == want[k].tolist(), k
    for k in ("sensitivity", "precision", "f1", "fp_per_image"):
        assert les["per_class"][k] == [None if np.isnan(v) else float(v) for v in want[k]], k
        kept = [v for v in les["per_class"][k][1:] if v is not None]
        assert les["mean"][k] == (sum(kept) / len(kept) if kept else None), k
    counts = torch.from_numpy(CO.overlap_counts(clean, masks.numpy(), 3)[0])
    assert rep["per_class"]["dice"] == SG.dice_per_class(counts).tolist() and rep["per_class"]["iou"] == SG.iou_per_class(counts).tolist()
    assert rep["mean"]["dice"] == SG.mean_dice(counts) and rep["pixel_accuracy"] == SG.pixel_accuracy(counts)
    sc, sv = ops.surface_stats(dev(clean), masks.to(DEV), torch.from_numpy(grid), 3, tolerances=(1.0, 2.0))      # the surface scores: on the cleaned map too
    acc = SG.SurfaceAccumulator(3, 2)
    for i in range(0, 12, 5):
        acc.update(SG.surface_metrics(sc[i:i + 5], sv[i:i + 5], grid[i:i + 5], (32, 32)))
    assert rep["per_class"]["hd95_mm"] == es._floats(acc.result()["hd95"]) and rep["per_class"]["surface_images"] == acc.result()["images"].tolist()

    # without any of the new flags: exactly the old key sets, and the scores of the unfiltered map
    plain = tmp_path / "plain.json"
    es.run(es.build_parser().parse_args(base + ["--out", str(plain)]))
    old = json.loads(plain.read_text())
    assert set(old) == OLD_KEYS
    assert set(old["per_class"]) == {"dice", "iou", "hd95_mm", "assd_mm", "nsd", "surface_images", "overlap_images"}
    assert set(old["mean"]) == {"dice", "iou", "hd95_mm", "assd_mm", "nsd", "classes"}
    counts = torch.from_numpy(CO.overlap_counts(pred, masks.numpy(), 3)[0])
    assert old["per_class"]["dice"] == SG.dice_per_class(counts).tolist() and old["mean"]["dice"] == SG.mean_dice(counts)
