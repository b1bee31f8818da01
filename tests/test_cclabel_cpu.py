"""CPU checks of the connected-component path: the oracle (tests/_cc_oracle.py) on hand-made maps with known answers, its run-based
labeller against its flood fill, dinox.segment.lesion_metrics / LesionAccumulator / min_component_px on hand-made numbers, every argument
refusal of ops.cc_label / cc_filter / lesion_counts and of the C entries (host checks, nothing is launched), and the new flags of
scripts/evaluate_segmentation.py."""
import importlib.util
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

import _cc_oracle as CO
from conftest import ROOT


def _one(rows):
    return np.array(rows, np.uint8)[None]


# ------------------------------------------------------------------------------------------ the oracle on maps with known answers
@pytest.mark.parametrize("label", (CO.label_flood, CO.label_runs))
def test_ring_of_three_by_three(label):
    m = _one([[1, 1, 1], [1, 0, 1], [1, 1, 1]])
    for conn in (4, 8):
        comp, area, ncomp = label(m, 2, conn)
        assert comp[0].tolist() == [[0, 0, 0], [0, 4, 0], [0, 0, 0]]
        assert area[0].tolist() == [[8, 0, 0], [0, 1, 0], [0, 0, 0]] and ncomp.tolist() == [[1, 1]]
    assert comp.dtype == np.int32 and area.dtype == np.int32 and ncomp.dtype == np.int64


@pytest.mark.parametrize("label", (CO.label_flood, CO.label_runs))
def test_two_diagonal_pixels(label):
    m = _one([[1, 0], [0, 1]])
    comp, area, ncomp = label(m, 2, 4)
    assert comp[0].tolist() == [[0, 1], [2, 3]] and area[0].tolist() == [[1, 1], [1, 1]] and ncomp.tolist() == [[2, 2]]
    comp, area, ncomp = label(m, 2, 8)
    assert comp[0].tolist() == [[0, 1], [1, 0]] and area[0].tolist() == [[2, 2], [0, 0]] and ncomp.tolist() == [[1, 1]]


@pytest.mark.parametrize("label", (CO.label_flood, CO.label_runs))
def test_four_pixel_corner_where_four_tiles_meet(label):
    m = np.zeros((1, 64, 64), np.uint8)
    m[0, 31, 31] = m[0, 32, 32] = 1                # one pixel in the first and one in the fourth of four 32 x 32 tiles
    m[0, 31, 32] = m[0, 32, 31] = 2                # and the other diagonal
    comp, area, ncomp = label(m, 3, 8)
    assert comp[0, 32, 32] == comp[0, 31, 31] == 31 * 64 + 31 and area[0, 31, 31] == 2
    assert comp[0, 32, 31] == comp[0, 31, 32] == 31 * 64 + 32 and area[0, 31, 32] == 2
    assert ncomp.tolist() == [[1, 1, 1]]           # the background stays one component around them (connectivity 8)
    comp, area, ncomp = label(m, 3, 4)
    assert ncomp.tolist() == [[1, 2, 2]] and comp[0, 32, 32] == 32 * 64 + 32 and area[0, 32, 32] == 1


def test_mask_and_values_outside_the_classes():
    m = _one([[1, 1, 1, 1], [0, 255, 0, 3]])
    mask = _one([[0, 255, 0, 0], [0, 0, 0, 255]])
    comp, area, ncomp = CO.label_flood(m, 2, 8, mask)
    assert comp[0].tolist() == [[0, -1, 2, 2], [4, -1, 6, -1]] and ncomp.tolist() == [[2, 2]]
    assert CO.bad_values(m, 2, mask) == 0 and CO.bad_values(m, 2) == 1 and CO.bad_values(m, 4) == 0


def _structured(H, W, rng):
    yy, xx = np.mgrid[:H, :W]
    out = [((yy + xx) % 2).astype(np.uint8), (yy == xx).astype(np.uint8), ((yy % 2 == 0) | (xx == 0)).astype(np.uint8)]
    snake = np.zeros((H, W), np.uint8)
    snake[::2] = 1
    snake[1::4, W - 1] = 1
    snake[3::4, 0] = 1
    out.append(snake)
    noise = rng.integers(0, 3, (H, W)).astype(np.uint8)
    noise[rng.random((H, W)) < 0.05] = 255
    out.append(noise)
    return np.stack(out)


def test_run_labeller_equals_flood_fill():
    rng = np.random.default_rng(5)
    for H, W in ((1, 1), (1, 9), (9, 1), (12, 17), (33, 40)):
        maps = _structured(H, W, rng)
        mask = (rng.random(maps.shape) < 0.1).astype(np.uint8) * 255
        for conn in (4, 8):
            for mk in (None, mask):
                a, b = CO.label_flood(maps, 3, conn, mk), CO.label_runs(maps, 3, conn, mk)
                assert all(np.array_equal(p, q) for p, q in zip(a, b)), (H, W, conn)
                assert (a[1].sum((1, 2)) == (a[0] >= 0).sum((1, 2))).all() and ((a[1] > 0).sum((1, 2)) == a[2].sum(1)).all()


def test_oracle_filter_and_match_on_hand_made_maps():
    lab = _one([[1, 1, 0, 1, 1], [0, 0, 0, 0, 0], [1, 0, 2, 2, 2]])
    assert CO.cc_filter(lab, 3, keep_largest=True)[0].tolist() == [[1, 1, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 2, 2, 2]]      # the tie: first root wins
    assert CO.cc_filter(lab, 3, min_px=[2])[0].tolist() == [[1, 1, 0, 1, 1], [0, 0, 0, 0, 0], [0, 0, 2, 2, 2]]
    assert CO.cc_filter(lab, 3, min_px=[3], keep_largest=True)[0].tolist() == [[0] * 5, [0] * 5, [0, 0, 2, 2, 2]]
    assert CO.cc_filter(lab, 3, min_px=[9], first_class=2)[0].tolist() == [[1, 1, 0, 1, 1], [0] * 5, [1, 0, 0, 0, 0]]
    gt = _one([[1, 1, 0, 0, 1], [0, 0, 0, 0, 0], [1, 0, 0, 2, 2]])
    pred = _one([[1, 0, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 2, 2, 2]])
    c = CO.lesion_counts(pred, gt, 3)
    assert c[0, 1].tolist() == [3, 1, 1, 1] and c[0, 2].tolist() == [1, 1, 1, 1]
    assert CO.lesion_counts(pred, gt, 3, overlap=(3, 4))[0].tolist() == [[1, 1, 1, 0], [3, 0, 1, 1], [1, 1, 1, 0]]
    counts, bad = CO.overlap_counts(pred, gt, 3)
    assert counts.tolist() == [[8, 1, 2], [11, 1, 3], [9, 4, 2]] and bad == 0


# ------------------------------------------------------------------------------------------ dinox.segment: metrics, accumulator, min_px
def _hand_counts():
    c = torch.zeros((2, 4, 4), dtype=torch.int64)
    c[0, 1], c[1, 1] = torch.tensor([3, 2, 4, 2]), torch.tensor([1, 1, 2, 1])        # class 1: 4 gt, 3 hit; 6 pred, 3 hit
    c[0, 2] = torch.tensor([2, 0, 0, 0])                                             # class 2: missed everywhere, never predicted
    c[1, 3] = torch.tensor([0, 0, 3, 0])                                             # class 3: only false positives
    return c                                                                         # class 0: nothing at all


def test_lesion_metrics_and_zero_denominators():
    from dinox.segment import lesion_metrics
    m = lesion_metrics(_hand_counts())
    assert m["images"] == 2 and m["sensitivity"].dtype == torch.float64
    assert m["sensitivity"][1] == 0.75 and m["precision"][1] == 0.5 and m["f1"][1] == pytest.approx(0.6) and m["fp_per_image"][1] == 1.5
    assert m["sensitivity"][2] == 0.0 and torch.isnan(m["precision"][2]) and torch.isnan(m["f1"][2]) and m["fp_per_image"][2] == 0.0
    assert torch.isnan(m["sensitivity"][3]) and m["precision"][3] == 0.0 and torch.isnan(m["f1"][3]) and m["fp_per_image"][3] == 1.5
    assert torch.isnan(m["sensitivity"][0]) and torch.isnan(m["precision"][0]) and torch.isnan(m["f1"][0]) and m["fp_per_image"][0] == 0.0
    assert m["n_gt"].tolist() == [0, 4, 2, 0] and m["n_gt_hit"].tolist() == [0, 3, 0, 0]
    assert m["n_pred"].tolist() == [0, 6, 0, 3] and m["n_pred_hit"].tolist() == [0, 3, 0, 0]
    hit_nothing = torch.tensor([[[2, 0, 2, 0]] * 2])                                  # P = R = 0: F1 has no value
    assert torch.isnan(lesion_metrics(hit_nothing)["f1"]).all()
    ref = CO.lesion_metrics(_hand_counts().numpy())
    for k in ("sensitivity", "precision", "f1", "fp_per_image"):
        assert np.array_equal(m[k].numpy(), ref[k], equal_nan=True)
    for bad in (torch.zeros((2, 4, 3), dtype=torch.int64), torch.zeros((4, 4), dtype=torch.int64), torch.zeros((2, 4, 4))):
        with pytest.raises(ValueError, match="lesion_metrics"):
            lesion_metrics(bad)


def test_lesion_accumulator():
    from dinox.segment import LesionAccumulator, lesion_metrics
    c = _hand_counts()
    acc = LesionAccumulator(4)
    for b in range(2):
        acc.update(c[b:b + 1])
    got, want = acc.result(), lesion_metrics(c)
    assert got["images"] == 2
    for k in want:
        if k != "images":
            assert torch.equal(torch.nan_to_num(got[k].double(), nan=-1.0), torch.nan_to_num(want[k].double(), nan=-1.0)), k
    empty = LesionAccumulator(3).result()
    assert empty["images"] == 0 and all(torch.isnan(empty[k]).all() for k in ("sensitivity", "precision", "f1", "fp_per_image"))
    with pytest.raises(ValueError, match="LesionAccumulator"):
        LesionAccumulator(3).update(c)


def test_min_px_conversion():
    from dinox.segment import min_component_px
    sp = torch.tensor([[0.5, 0.5], [0.7, 1.3], [2.0, 1.0]], dtype=torch.float32)
    assert min_component_px(1.0, sp, 3) == [4, math.ceil(1.0 / (float(sp[1, 0]) * float(sp[1, 1]))), 1]
    assert min_component_px(1.0, sp, 3) == CO.min_px(1.0, sp.numpy())
    assert min_component_px(0.0, sp, 3) == [0, 0, 0]
    assert min_component_px(10.0, None, 2) == [10, 10] and min_component_px(2.5, (1.0, 1.0), 2) == [3, 3]
    assert min_component_px(1.0, [[0.25, 0.25]], 1) == [16]                          # exactly 16 pixels reach 1 mm^2
    for kw in (dict(min_area_mm2=-1.0), dict(min_area_mm2=float("nan")), dict(spacing=[[1.0, 0.0]] * 3), dict(spacing=[[1.0, 1.0]] * 2),
               dict(min_area_mm2=1e30)):
        args = dict(min_area_mm2=1.0, spacing=sp, B=3)
        args.update(kw)
        with pytest.raises(ValueError):
            min_component_px(**args)


# ------------------------------------------------------------------------------------------ ops: refusals
U8 = torch.zeros((2, 8, 8), dtype=torch.uint8)
COMMON = [
    (dict(labels=U8.float()), "must be uint8"),
    (dict(labels=U8[0]), "must be uint8"),
    (dict(labels=torch.zeros((1, 1025, 4), dtype=torch.uint8)), "1024"),
    (dict(labels=torch.zeros((0, 4, 4), dtype=torch.uint8)), "B >= 1"),
    (dict(num_classes=1), "num_classes"),
    (dict(num_classes=65), "num_classes"),
    (dict(num_classes=2.0), "num_classes"),
    (dict(num_classes=True), "num_classes"),
    (dict(connectivity=6), "connectivity"),
    (dict(connectivity=8.0), "connectivity"),
]


def _refused(fn, name, base, cases):
    for kw, msg in cases:
        args = dict(base)
        args.update(kw)
        with pytest.raises(ValueError, match=msg) as e:
            fn(**args)
        assert name in str(e.value), (kw, str(e.value))
    with pytest.raises(RuntimeError, match="CUDA/HIP device"):      # argument errors first, then: no CPU path
        fn(**base)


def test_cc_label_refuses_bad_arguments():
    from dinox import ops
    _refused(ops.cc_label, "cc_label", dict(labels=U8, num_classes=3), COMMON + [
        (dict(mask=U8.int()), "mask must be uint8"), (dict(mask=U8[:, :4]), "differ in shape")])


def test_cc_filter_refuses_bad_arguments():
    from dinox import ops
    _refused(ops.cc_filter, "cc_filter", dict(labels=U8, num_classes=3), COMMON + [
        (dict(mask=U8[:1]), "differ in shape"), (dict(targets=U8.long()), "targets must be uint8"), (dict(targets=U8[:, :, :4]), "differ in shape"),
        (dict(first_class=-1), "first_class"), (dict(first_class=4), "first_class"), (dict(first_class=1.0), "first_class"),
        (dict(keep_largest="yes"), "keep_largest"),
        (dict(min_px=1.5), "min_px"), (dict(min_px=[1]), "min_px"), (dict(min_px=[1, -1]), "min_px"), (dict(min_px=[1, 2.0]), "min_px"),
        (dict(min_px=True), "min_px"), (dict(min_px=torch.ones(2)), "min_px"), (dict(min_px=torch.ones(3, dtype=torch.int32)), "min_px"),
        (dict(min_px=torch.tensor([1, -2])), "min_px"), (dict(min_px=[1, 1 << 31]), "min_px")])


def test_lesion_counts_refuses_bad_arguments():
    from dinox import ops
    cases = [(dict(pred=kw["labels"], labels=kw["labels"]) if "labels" in kw else kw, msg) for kw, msg in COMMON]
    _refused(ops.lesion_counts, "lesion_counts", dict(pred=U8, labels=U8, num_classes=3), cases + [
        (dict(labels=U8.float()), "labels must be uint8"), (dict(labels=U8[:, :4]), "differ in shape"),
        (dict(overlap=0.5), "overlap"), (dict(overlap=(1, 0)), "overlap"), (dict(overlap=(2, 1)), "overlap"), (dict(overlap=(-1, 2)), "overlap"),
        (dict(overlap=(0.5, 1)), "overlap"), (dict(overlap=(1, 1 << 20)), "overlap"), (dict(overlap=(1, 2, 3)), "overlap"),
        (dict(min_px=[1, 2, 3]), "min_px"), (dict(min_px="a"), "min_px")])


def test_c_entries_check_their_arguments_before_any_launch():
    from dinox import _lib
    lib = _lib.lib
    assert lib.dinox_cc_ws_bytes(3, 300, 70, 5) == 8 * 3 * 300 * 70 + 8 * 3 * 5
    assert lib.dinox_cc_ws_bytes(2047, 1024, 1024, 2) > 0
    for sizes in ((0, 8, 8, 2), (1, 0, 8, 2), (1, 8, 1025, 2), (1, 1025, 8, 2), (1, 8, 8, 1), (1, 8, 8, 65), (2048, 1024, 1024, 2), (1 << 31, 1, 1, 2),
                  (1 << 40, 1, 1, 2)):
        assert lib.dinox_cc_ws_bytes(*sizes) == 0, sizes
    p = 0x1000                                     # never dereferenced: every call below is refused on the host
    sizes = [(dict(H=0), "H=0"), (dict(W=1025), "W=1025"), (dict(C=1), "C=1"), (dict(C=65), "C=65"), (dict(B=0), "B=0"),
             (dict(B=2048, H=1024, W=1024), "B=2048")]
    ok = dict(B=1, H=8, W=8, C=2)

    def label(a, conn=8, labels=p, bad=p):
        return lib.dinox_cc_label(labels, None, p, p, p, bad, p, a["B"], a["H"], a["W"], a["C"], conn, None)

    def filt(a, c0=1, y=None, counts=None, out=p):
        return lib.dinox_cc_filter(p, p, p, None, y, out, counts, p, a["B"], a["H"], a["W"], a["C"], c0, 0, None)

    def match(a, tn=0, td=1, gt=p):
        return lib.dinox_cc_match(p, p, p, gt, p, p, None, p, p, a["B"], a["H"], a["W"], a["C"], tn, td, None)

    for name, call in (("cc_label", label), ("cc_filter", filt), ("cc_match", match)):
        for kw, msg in sizes:
            assert call(dict(ok, **kw)) == -1 and msg in _lib.last_error() and name in _lib.last_error(), (name, kw, _lib.last_error())
    for conn in (0, 6, 9):
        assert label(ok, conn=conn) == -1 and f"connectivity={conn}" in _lib.last_error()
    assert label(ok, labels=None) == -1 and "null pointer" in _lib.last_error()
    assert label(ok, bad=None) == -1 and "null pointer" in _lib.last_error()
    assert filt(ok, out=None) == -1 and "null pointer" in _lib.last_error()
    assert filt(ok, y=p) == -1 and "both or neither" in _lib.last_error()
    assert filt(ok, counts=p) == -1 and "both or neither" in _lib.last_error()
    for c0 in (-1, 3):
        assert filt(ok, c0=c0) == -1 and f"c0={c0}" in _lib.last_error()
    assert match(ok, gt=None) == -1 and "null pointer" in _lib.last_error()
    for tn, td in ((-1, 2), (3, 2), (0, 0), (1, 1 << 20)):
        assert match(ok, tn=tn, td=td) == -1 and f"overlap {tn}/{td}" in _lib.last_error()


# ------------------------------------------------------------------------------------------ scripts/evaluate_segmentation.py
def _script():
    if "evaluate_segmentation" in sys.modules:
        return sys.modules["evaluate_segmentation"]
    spec = importlib.util.spec_from_file_location("evaluate_segmentation", os.path.join(ROOT, "dino-x_amd", "scripts", "evaluate_segmentation.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def test_parser_defaults_of_the_new_flags():
    es = _script()
    a = es.build_parser().parse_args(["--backbone", "b", "--segmenter", "s"])
    assert (a.lesion_metrics, a.lesion_overlap, a.connectivity, a.keep_largest, a.min_component_mm2) == (False, 0.0, 8, False, 0.0)
    a = es.build_parser().parse_args(["--backbone", "b", "--segmenter", "s", "--lesion-metrics", "--lesion-overlap", "0.25", "--connectivity", "4",
                                      "--keep-largest", "--min-component-mm2", "2.5"])
    assert (a.lesion_metrics, a.lesion_overlap, a.connectivity, a.keep_largest, a.min_component_mm2) == (True, 0.25, 4, True, 2.5)
    with pytest.raises(SystemExit):
        es.build_parser().parse_args(["--backbone", "b", "--segmenter", "s", "--connectivity", "6"])


def test_script_refuses_bad_values_of_the_new_flags(tmp_path, capsys):
    es = _script()
    seg = tmp_path / "seg"
    seg.mkdir()
    (seg / "finetune_config.json").write_text(json.dumps({"task": "segmentation", "num_classes": 3, "rank": 0}))
    base = ["--backbone", "b", "--segmenter", str(seg), "--synthetic", "8"]
    for extra, msg in ((["--lesion-overlap", "1.5"], "--lesion-overlap"), (["--lesion-overlap", "-0.1"], "--lesion-overlap"),
                       (["--lesion-overlap", "nan"], "--lesion-overlap"), (["--min-component-mm2", "-1"], "--min-component-mm2"),
                       (["--min-component-mm2", "inf"], "--min-component-mm2"), (["--min-component-mm2", "nan"], "--min-component-mm2")):
        with pytest.raises(SystemExit) as e:
            es.run(es.build_parser().parse_args(base + extra))
        assert msg in str(e.value.code) + capsys.readouterr().err, extra


def test_lesion_report_layout():
    es = _script()
    from dinox.segment import lesion_metrics
    rep = es.lesion_report(lesion_metrics(_hand_counts()), 8, (250, 1000), 2.5)
    assert set(rep) == {"connectivity", "overlap", "min_area_mm2", "images", "per_class", "mean"}
    assert set(rep["per_class"]) == {"sensitivity", "precision", "f1", "fp_per_image", "n_gt", "n_gt_hit", "n_pred", "n_pred_hit"}
    assert rep["overlap"] == "250/1000" and rep["connectivity"] == 8 and rep["min_area_mm2"] == 2.5 and rep["images"] == 2
    assert rep["per_class"]["sensitivity"] == [None, 0.75, 0.0, None] and rep["per_class"]["n_pred"] == [0, 6, 0, 3]
    assert rep["mean"] == {"sensitivity": 0.375, "precision": 0.25, "f1": pytest.approx(0.6), "fp_per_image": 1.0, "classes": 1}
    json.dumps(rep)
