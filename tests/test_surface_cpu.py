"""CPU checks of the surface-distance path: the float64 oracle (tests/_surface_oracle.py) against cases whose answers can be written down
and against scipy.ndimage, dinox.segment.surface_metrics / SurfaceAccumulator on hand-made counts, the argument refusals of
ops.surface_stats and of the C entry (host checks, nothing is launched), and scripts/evaluate_segmentation.py's parser and refusals."""
import importlib.util
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

import _surface_oracle as SO
from conftest import ROOT


def _maps(H, W):
    return np.zeros((1, H, W), np.uint8), np.zeros((1, H, W), np.uint8)


# ------------------------------------------------------------------------------------------ the oracle on cases with known answers
def test_single_pixel_against_single_pixel():
    pred, gt = _maps(7, 9)
    pred[0, 1, 2], gt[0, 5, 8] = 1, 1
    D = SO.Distances(pred, gt, [[0.5, 2.0]], 2)
    want = math.hypot(0.5 * 4, 2.0 * 6)
    counts, values, _ = D.stats((12.0, 13.0), (95, 100))
    assert counts[0, 1].tolist() == [[1, 0, 1], [1, 0, 1]]
    assert np.allclose(values[0, 1], [[want] * 3] * 2, rtol=1e-15)
    assert D.min_gap((12.0,))[0] == pytest.approx((want - 12.0) / 12.0)


def test_two_concentric_squares():
    pred, gt = _maps(20, 20)
    gt[0, 4:16, 4:16] = 1                      # 12 x 12: border ring of 44 pixels
    pred[0, 6:14, 6:14] = 1                    # 8 x 8 inside it: ring of 28, every ring pixel 2 rows or columns from the outer ring
    D = SO.Distances(pred, gt, [[1.0, 1.0]], 2)
    ag, ga = D.d[0][1]
    assert len(ag) == 28 and len(ga) == 44 and np.all(ag == 2.0)
    assert ga.min() == 2.0 and ga.max() == pytest.approx(math.sqrt(8.0))      # the outer corners see the inner corners diagonally
    assert np.isclose(ga.sum(), 32 * 2.0 + 8 * math.sqrt(5.0) + 4 * math.sqrt(8.0))      # beside each corner: one across, two up
    counts, values, _ = D.stats((1.5, 2.5), (95, 100))
    assert counts[0, 1].tolist() == [[28, 0, 28], [44, 0, 40]]
    assert values[0, 1, 1, 2] == pytest.approx(math.sqrt(8.0))                # k = ceil(44 * 0.95) = 42: past the 32 + 8 shorter ones
    assert D.stats((1.5,), (1, 2))[1][0, 1, 1, 2] == 2.0 and D.stats((1.5,), (10, 11))[1][0, 1, 1, 2] == pytest.approx(math.sqrt(5.0))


def test_object_touching_the_edge_and_full_image_object():
    X = np.zeros((6, 8), bool)
    X[0:3, 0:4] = True
    b = SO.border(X)
    assert b.sum() == 10 and not b[1, 1] and not b[1, 2] and b[0, 1] and b[1, 0]          # the image edge counts as outside
    full = SO.border(np.ones((5, 7), bool))
    assert full.sum() == 2 * 5 + 2 * 7 - 4 and not full[1:-1, 1:-1].any()
    assert SO.border(np.ones((1, 1), bool)).all() and SO.border(np.ones((1, 5), bool)).all()


def test_identical_maps_and_ignored_pixels():
    rng = np.random.default_rng(3)
    gt = rng.integers(0, 3, (2, 12, 10)).astype(np.uint8)
    D = SO.Distances(gt.copy(), gt, [[0.7, 1.3], [1.0, 1.0]], 3)
    counts, values, bound = D.stats((1.0,), (95, 100))
    assert not values.any() and not bound.any() and (counts[..., 0] == counts[..., 1]).all() and counts[..., 0].min() > 0
    m = SO.metrics(counts, values, D.spacing, (12, 10))
    assert not m["hd95"].any() and not m["assd"].any() and (m["nsd"] == 1.0).all()
    pred = gt.copy()
    gt[0, 3:6, :] = 255                                                        # ignored pixels are in neither set
    A, G = SO.sets(pred[0], gt[0], 1)
    assert not A[3:6].any() and not G[3:6].any() and np.array_equal(A, G)


def test_oracle_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(11)
    for (H, W), (sy, sx) in (((33, 17), (0.7, 1.3)), ((24, 40), (2.5, 0.6))):
        pred = (ndi.uniform_filter(rng.random((H, W)), 5) > 0.5).astype(np.uint8)
        gt = (ndi.uniform_filter(rng.random((H, W)), 5) > 0.5).astype(np.uint8)
        for c in (0, 1):
            A, G = SO.sets(pred, gt, c)
            bA, bG = A & ~ndi.binary_erosion(A), G & ~ndi.binary_erosion(G)
            assert np.array_equal(bA, SO.border(A)) and np.array_equal(bG, SO.border(G))
            assert bA.any() and bG.any()
            want = ndi.distance_transform_edt(~bG, sampling=(sy, sx))[bA]
            got = SO.directed(np.argwhere(bA), np.argwhere(bG), sy, sx)
            assert np.allclose(got, want, rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------------------------------ dinox.segment.surface_metrics / SurfaceAccumulator
def _hand_counts():
    """B = 2, C = 4, T = 2.  Image 0: class 0 ordinary, class 1 only in pred, class 2 only in gt, class 3 absent.  Image 1: class 0 only."""
    counts = torch.zeros((2, 4, 2, 3), dtype=torch.int64)
    values = torch.zeros((2, 4, 2, 3), dtype=torch.float32)
    counts[0, 0, 0], counts[0, 0, 1] = torch.tensor([20, 10, 15]), torch.tensor([30, 12, 30])
    values[0, 0, 0], values[0, 0, 1] = torch.tensor([40.0, 5.0, 4.0]), torch.tensor([45.0, 7.5, 3.0])
    counts[0, 1, 0, 0] = 9                       # hallucinated
    counts[0, 2, 1, 0] = 4                       # missed
    counts[1, 0, 0], counts[1, 0, 1] = torch.tensor([10, 10, 10]), torch.tensor([10, 10, 10])
    return counts, values


def test_surface_metrics_and_both_empty_class_branches():
    from dinox.segment import surface_metrics
    counts, values = _hand_counts()
    spacing = torch.tensor([[0.5, 2.0], [1.0, 1.0]])
    m = surface_metrics(counts, values, spacing, (30, 40))
    diag = math.hypot(0.5 * 30, 2.0 * 40)
    assert m["hd95"].dtype == torch.float64 and m["nsd"].shape == (2, 4, 2)
    assert m["hd95"][0, 0] == 4.0 and m["hd"][0, 0] == 7.5 and m["assd"][0, 0] == pytest.approx(85.0 / 50.0)
    assert m["nsd"][0, 0].tolist() == pytest.approx([22 / 50, 45 / 50])
    for c in (1, 2):                             # exactly one border empty: the diagonal, NSD 0
        assert m["hd95"][0, c] == pytest.approx(diag) and m["hd"][0, c] == pytest.approx(diag) and m["assd"][0, c] == pytest.approx(diag)
        assert m["nsd"][0, c].tolist() == [0.0, 0.0]
    assert all(torch.isnan(m[k][0, 3]).all() for k in m) and all(torch.isnan(m[k][1, 1:]).all() for k in m)      # absent: NaN
    assert m["hd95"][1, 0] == 0.0 and m["nsd"][1, 0].tolist() == [1.0, 1.0]
    ref = SO.metrics(counts.numpy(), values.numpy(), spacing.numpy(), (30, 40))
    for k in m:
        assert np.allclose(m[k].numpy(), ref[k], rtol=1e-15, equal_nan=True)
    with pytest.raises(ValueError, match="counts must be"):
        surface_metrics(counts[:, :, 0], values, spacing, (30, 40))
    with pytest.raises(ValueError, match="spacing must be"):
        surface_metrics(counts, values, spacing[:1], (30, 40))


def test_accumulator_means_and_image_counts():
    from dinox.segment import SurfaceAccumulator, surface_metrics
    counts, values = _hand_counts()
    spacing = torch.tensor([[0.5, 2.0], [1.0, 1.0]])
    acc = SurfaceAccumulator(4, 2)
    for b in range(2):                           # one image at a time: a stream of batches
        acc.update(surface_metrics(counts[b:b + 1], values[b:b + 1], spacing[b:b + 1], (30, 40)))
    res = acc.result()
    diag = math.hypot(0.5 * 30, 2.0 * 40)
    assert res["images"].tolist() == [2, 1, 1, 0]
    assert res["hd95"][0] == pytest.approx(2.0) and res["assd"][0] == pytest.approx(0.85) and res["nsd"][0].tolist() == pytest.approx([0.72, 0.95])
    assert res["hd95"][1] == pytest.approx(diag) and res["nsd"][2].tolist() == [0.0, 0.0]
    assert torch.isnan(res["hd95"][3]) and torch.isnan(res["nsd"][3]).all()
    whole = SurfaceAccumulator(4, 2)
    whole.update(surface_metrics(counts, values, spacing, (30, 40)))
    assert all(torch.equal(torch.nan_to_num(whole.result()[k].double(), nan=-1.0), torch.nan_to_num(res[k].double(), nan=-1.0)) for k in res)
    with pytest.raises(ValueError, match="SurfaceAccumulator"):
        SurfaceAccumulator(3, 2).update(surface_metrics(counts, values, spacing, (30, 40)))


def test_integer_rank():
    """k = ceil(n q_num / q_den) in integers: n = 20 at 95/100 is the 19th smallest, not the 20th."""
    pred, gt = _maps(3, 40)
    pred[0, 1, :20] = 1                          # 20 border pixels in a row
    gt[0, 1, 39] = 1
    D = SO.Distances(pred, gt, [[1.0, 1.0]], 2)
    assert len(D.d[0][1][0]) == 20
    assert D.stats((1.0,), (95, 100))[1][0, 1, 0, 2] == 38.0 and D.stats((1.0,), (1, 1))[1][0, 1, 0, 2] == 39.0
    assert D.stats((1.0,), (1, 2))[1][0, 1, 0, 2] == 29.0


# ------------------------------------------------------------------------------------------ ops.surface_stats and the C entry: refusals
def test_surface_stats_refuses_bad_arguments():
    from dinox import ops
    u8 = torch.zeros((2, 8, 8), dtype=torch.uint8)
    sp = torch.ones((2, 2))
    bad = [
        (dict(pred=u8.float()), "pred must be uint8"),
        (dict(labels=u8[0]), "labels must be uint8"),
        (dict(labels=u8[:, :4]), "differ in shape"),
        (dict(pred=torch.zeros((1, 1025, 4), dtype=torch.uint8), labels=torch.zeros((1, 1025, 4), dtype=torch.uint8), spacing=sp[:1]), "1024"),
        (dict(num_classes=1), "num_classes"),
        (dict(num_classes=65), "num_classes"),
        (dict(num_classes=2.0), "num_classes"),
        (dict(tolerances=()), "tolerances"),
        (dict(tolerances=(1.0,) * 9), "tolerances"),
        (dict(tolerances=(-1.0,)), "tolerances"),
        (dict(tolerances=(float("inf"),)), "tolerances"),
        (dict(q=(0, 100)), "q must be"),
        (dict(q=(101, 100)), "q must be"),
        (dict(q=(0.95, 1)), "q must be"),
        (dict(q=95), "q must be"),
    ]
    for kw, msg in bad:
        args = dict(pred=u8, labels=u8, spacing=sp, num_classes=3)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            ops.surface_stats(**args)
    with pytest.raises(RuntimeError, match="CUDA/HIP device"):      # argument errors first, then: no CPU path
        ops.surface_stats(u8, u8, sp, 3)


def test_c_entry_checks_its_arguments_before_any_launch():
    from dinox import _lib
    lib, f32 = _lib.lib, _lib.f32
    assert lib.dinox_surface_ws_bytes(3, 300, 70, 5) == 12 * 3 * 5 * 300 * 70
    for sizes in ((0, 8, 8, 2), (1, 0, 8, 2), (1, 8, 1025, 2), (1, 8, 8, 1), (1, 8, 8, 65), (1 << 20, 1024, 8, 64)):
        assert lib.dinox_surface_ws_bytes(*sizes) == 0
    tol = (f32 * 2)(1.0, 2.0)
    p = 0x1000                                   # never dereferenced: every call below is refused on the host
    ok = dict(B=1, H=8, W=8, C=2, T=2, qn=95, qd=100)
    for kw, msg in ((dict(H=0), "H=0"), (dict(W=1025), "W=1025"), (dict(C=1), "C=1"), (dict(C=65), "C=65"), (dict(B=0), "B=0"), (dict(T=0), "T=0"),
                    (dict(T=9), "T=9"), (dict(qn=0), "quantile"), (dict(qn=3, qd=2), "quantile")):
        a = dict(ok, **kw)
        rc = lib.dinox_surface_stats(p, p, p, tol, p, p, p, p, a["B"], a["H"], a["W"], a["C"], a["T"], a["qn"], a["qd"], None)
        assert rc == -1 and msg in _lib.last_error(), (kw, _lib.last_error())
    assert lib.dinox_surface_stats(p, p, p, (f32 * 1)(-0.5), p, p, p, p, 1, 8, 8, 2, 1, 95, 100, None) == -1 and "tolerance 0" in _lib.last_error()
    assert lib.dinox_surface_stats(p, None, p, tol, p, p, p, p, 1, 8, 8, 2, 2, 95, 100, None) == -1 and "null pointer" in _lib.last_error()


# ------------------------------------------------------------------------------------------ scripts/evaluate_segmentation.py
def _script():
    scripts = os.path.join(ROOT, "dino-x_amd", "scripts")
    if "evaluate_segmentation" in sys.modules:
        return sys.modules["evaluate_segmentation"]
    spec = importlib.util.spec_from_file_location("evaluate_segmentation", os.path.join(scripts, "evaluate_segmentation.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def test_parser_defaults():
    es = _script()
    a = es.build_parser().parse_args(["--backbone", "b", "--segmenter", "s"])
    assert (a.device, a.val_csv, a.synthetic, a.data_root, a.input_format, a.window_level, a.window_width) == ("cuda", None, 0, None, "hu16_png", 40.0, 400.0)
    assert (a.batch_size, a.no_amp, a.tolerance_mm, str(a.out), a.seed) == (32, False, None, "seg_eval.json", 0)
    a = es.build_parser().parse_args(["--backbone", "b", "--segmenter", "s", "--tolerance-mm", "0.5", "--tolerance-mm", "3", "--synthetic", "8", "--no-amp"])
    assert a.tolerance_mm == [0.5, 3.0] and a.synthetic == 8 and a.no_amp
    with pytest.raises(SystemExit):
        es.build_parser().parse_args(["--backbone", "b"])          # --segmenter is required


def test_script_refusals(tmp_path, capsys):
    es = _script()

    def refused(argv):
        with pytest.raises(SystemExit) as e:
            es.run(es.build_parser().parse_args(argv))
        return str(e.value.code) + capsys.readouterr().err

    seg = tmp_path / "seg"
    seg.mkdir()
    (seg / "finetune_config.json").write_text(json.dumps({"task": "segmentation", "num_classes": 3, "rank": 0}))
    assert "no CPU compute path" in refused(["--backbone", "b", "--segmenter", str(seg), "--synthetic", "8", "--device", "cpu"])
    assert "--val-csv is required" in refused(["--backbone", "b", "--segmenter", str(seg)])
    assert "no such file" in refused(["--backbone", "b", "--segmenter", str(seg), "--val-csv", str(tmp_path / "missing.csv")])
    assert "finetune_config.json" in refused(["--backbone", "b", "--segmenter", str(tmp_path), "--synthetic", "8"])
    other = tmp_path / "cls"
    other.mkdir()
    (other / "finetune_config.json").write_text(json.dumps({"task": "classification"}))
    assert "is not 'segmentation'" in refused(["--backbone", "b", "--segmenter", str(other), "--synthetic", "8"])
    assert "--tolerance-mm" in refused(["--backbone", "b", "--segmenter", str(seg), "--synthetic", "8", "--tolerance-mm", "-1"])


def test_resize_factors_follow_the_centre_crop():
    es = _script()
    assert es.resize_factors(512, 512, 224) == (512 / 224, 512 / 224)
    fy, fx = es.resize_factors(300, 400, 224)    # the shorter side goes to 224, the longer to round(400 * 224 / 300) = 299
    assert fy == 300 / 224 and fx == 400 / 299
    assert es.resize_factors(32, 32, 32) == (1.0, 1.0)
