"""CPU tests of the 3-D surface-distance path: the float64 oracle (tests/_surface3d_oracle.py) on hand-made volumes with known answers,
the workspace formula and every host refusal of the two C entries (nothing is launched), the argument errors of ops.surface_stats_3d,
dinox.segment.surface_metrics_3d on fabricated outputs, and the new flags of scripts/segment_volume.py."""
import ctypes
import importlib.util
import math
import os
import sys

import numpy as np
import pytest
import torch

import _surface3d_oracle as SO
from conftest import ROOT

SP = (2.5, 0.7, 1.3)
SP64 = np.asarray(SP, dtype=np.float32).astype(np.float64)


def _empty(shape=(5, 6, 7)):
    return np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)


# ------------------------------------------------------------------------------------------ the oracle on known answers
@pytest.mark.parametrize("off", ((1, 0, 0), (0, 2, 0), (0, 0, 3), (2, -1, 3), (-1, 3, -2)))
def test_oracle_two_single_voxels(off):
    pred, gt = _empty()
    gt[2, 2, 3] = 1
    pred[2 + off[0], 2 + off[1], 3 + off[2]] = 1
    D = SO.Distances(pred, gt, SP, 2)
    want = math.sqrt(sum((s * o) ** 2 for s, o in zip(SP64, off)))
    assert D.d[1][0].tolist() == pytest.approx([want], rel=1e-15) and D.d[1][1].tolist() == pytest.approx([want], rel=1e-15)
    counts, values, bound = D.stats((want * 0.99, want * 1.01))
    assert counts[1].tolist() == [[1, 0, 1], [1, 0, 1]]
    assert values[1].ravel().tolist() == pytest.approx([want] * 6, rel=1e-15)
    assert bound[1, 0, 1] == SO.REL * values[1, 0, 1] and SO.REL == 4 * 2.0 ** -24
    m = SO.metrics(counts, values, SP64, pred.shape)
    assert m["hd95"].shape == (1, 2) and m["nsd"].shape == (1, 2, 2)
    assert m["hd95"][0, 1] == pytest.approx(want) and m["assd"][0, 1] == pytest.approx(want) and m["nsd"][0, 1].tolist() == [0.0, 1.0]


def test_oracle_solid_cube_has_26_border_voxels():
    pred, gt = _empty((7, 7, 7))
    gt[2:5, 2:5, 2:5] = 1
    pred[2:5, 2:5, 2:5] = 1
    B = SO.border(gt == 1)
    assert B.sum() == 26 and not B[3, 3, 3]
    D = SO.Distances(pred, gt, SP, 2)
    assert len(D.d[1][0]) == 26 and not D.d[1][0].any() and not D.d[1][1].any()
    # the background: the volume's faces and the shell around the cube; a cube at the wall keeps its wall voxels as border
    assert SO.border(gt == 0).sum() == 7 ** 3 - 5 ** 3 + 6 * 9
    wall = np.zeros((4, 4, 4), bool)
    wall[:3, :3, :3] = True
    assert SO.border(wall).sum() == 26 and not SO.border(wall)[1, 1, 1]


def test_oracle_one_slice_is_all_border():
    pred, gt = _empty((1, 6, 7))
    gt[0, 1:5, 1:6] = 1                                       # a 4 x 5 rectangle: 14 border pixels in 2-D, all 20 voxels in 3-D
    pred[0, 1:5, 2:7] = 1
    assert SO.border(gt == 1).sum() == 20 and SO.border(gt == 0).sum() == 22
    D = SO.Distances(pred, gt, SP, 2)
    assert len(D.d[1][0]) == 20 and D.d[1][0].max() == pytest.approx(SP64[2]) and (D.d[1][0] == 0).sum() == 16


def test_oracle_one_sided_and_absent_classes():
    pred, gt = _empty()
    pred[1, 1, 1] = 1                                         # only in pred
    gt[3, 3, 3] = 2                                           # only in gt; class 3 in neither
    D = SO.Distances(pred, gt, SP, 4)
    counts, values, bound = D.stats((1.0, 2.0))
    assert counts[1].tolist() == [[1, 0, 0], [0, 0, 0]] and counts[2].tolist() == [[0, 0, 0], [1, 0, 0]] and not counts[3].any()
    assert not values[1:].any() and not bound[1:].any()
    assert D.min_gap((1.0, 2.0)) > 0
    m = SO.metrics(counts, values, SP64, pred.shape)
    diag = math.sqrt((SP64[0] * 5) ** 2 + (SP64[1] * 6) ** 2 + (SP64[2] * 7) ** 2)
    for k in ("hd95", "hd", "assd"):
        assert m[k][0, 1] == pytest.approx(diag) and m[k][0, 2] == pytest.approx(diag) and np.isnan(m[k][0, 3])
    assert m["nsd"][0, 1].tolist() == [0, 0] and m["nsd"][0, 2].tolist() == [0, 0] and np.isnan(m["nsd"][0, 3]).all()


def test_oracle_ignored_voxels_cut_an_object():
    pred, gt = _empty((5, 5, 9))
    gt[1:4, 1:4, 1:8] = 1
    pred[1:4, 1:4, 1:8] = 1
    gt[:, :, 4] = 255                                         # a wall of ignored voxels through the middle
    A, G = SO.sets(pred, gt, 1)
    assert not A[:, :, 4].any() and not G[:, :, 4].any() and np.array_equal(A, G)
    B = SO.border(G)
    assert B[2, 2, 3] and B[2, 2, 5] and not B[2, 2, 2] and B.sum() == 2 * 27 - 2      # two 3 x 3 x 3 halves, each with one inner voxel
    D = SO.Distances(pred, gt, SP, 2)
    assert not D.d[1][0].any() and len(D.d[1][0]) == 52
    assert not SO.sets(pred, gt, 0)[0][:, :, 4].any()         # ignored voxels are in no class's set, the background's included


# ------------------------------------------------------------------------------------------ the C entries: workspace and refusals
def test_workspace_formula():
    from dinox import _lib
    lib = _lib.lib
    assert lib.dinox_surface3d_ws_bytes(9, 33, 17, 5) == 12 * 9 * 33 * 17 + 8 * 9 + 8320
    assert lib.dinox_surface3d_ws_bytes(256, 224, 224, 3) == 12 * 256 * 224 * 224 + 8 * 256 + 8320
    assert lib.dinox_surface3d_ws_bytes(1024, 1024, 1024, 64) == 12 * (1 << 30) + 8 * 1024 + 8320 <= 20 * (1 << 30)
    assert lib.dinox_surface3d_ws_bytes(9, 33, 17, 2) == lib.dinox_surface3d_ws_bytes(9, 33, 17, 64)        # C does not enter
    for sizes in ((0, 8, 8, 2), (8, 0, 8, 2), (8, 8, 0, 2), (1025, 8, 8, 2), (8, 1025, 8, 2), (8, 8, 1025, 2), (8, 8, 8, 1), (8, 8, 8, 65),
                  (-1, 8, 8, 2), (1 << 40, 1, 1, 2)):
        assert lib.dinox_surface3d_ws_bytes(*sizes) == 0, sizes


def test_c_entry_checks_its_arguments_before_any_launch():
    from dinox import _lib
    lib = _lib.lib
    p = 0x1000                                                # never dereferenced: every call below is refused on the host
    sp_ok, tol_ok = (ctypes.c_float * 3)(2.5, 0.7, 1.3), (ctypes.c_float * 8)(*([1.0] * 8))

    def call(pred=p, gt=p, sp=sp_ok, tol=tol_ok, counts=p, values=p, bad=p, ws=p, Z=4, H=8, W=8, C=3, T=2, qn=95, qd=100):
        rc = lib.dinox_surface3d_stats(pred, gt, sp, tol, counts, values, bad, ws, Z, H, W, C, T, qn, qd, None)
        return rc, _lib.last_error()

    for name in ("pred", "gt", "sp", "tol", "counts", "values", "bad", "ws"):
        rc, msg = call(**{name: None})
        assert rc == -1 and "surface3d_stats: null pointer" in msg, (name, msg)
    for kw, want in ((dict(Z=0), "Z=0"), (dict(Z=1025), "Z=1025"), (dict(H=0), "H=0"), (dict(H=1025), "H=1025"), (dict(W=0), "W=0"),
                     (dict(W=1025), "W=1025"), (dict(C=1), "C=1"), (dict(C=65), "C=65"), (dict(T=0), "T=0"), (dict(T=9), "T=9"),
                     (dict(qn=0), "quantile 0/100"), (dict(qn=101), "quantile 101/100"), (dict(qn=-1, qd=-1), "quantile -1/-1")):
        rc, msg = call(**kw)
        assert rc == -1 and "surface3d_stats" in msg and want in msg, (kw, msg)
    for bad_tol in (-1.0, float("nan"), float("inf")):
        rc, msg = call(tol=(ctypes.c_float * 2)(1.0, bad_tol))
        assert rc == -1 and "tolerance 1 is" in msg, msg
    for axis in range(3):
        for bad_sp in (0.0, -1.0, float("nan"), float("inf")):
            v = [2.5, 0.7, 1.3]
            v[axis] = bad_sp
            rc, msg = call(sp=(ctypes.c_float * 3)(*v))
            assert rc == -1 and f"spacing {axis} is" in msg, msg


def test_abi_version_is_unchanged():
    from dinox import _lib
    assert _lib.lib.dinox_version() == 3
    assert "dinox_surface3d_stats" in _lib.SIGNATURES and "dinox_surface3d_ws_bytes" in _lib.SIGNATURES


# ------------------------------------------------------------------------------------------ ops.surface_stats_3d
U8 = torch.zeros((2, 8, 8), dtype=torch.uint8)


def test_surface_stats_3d_refuses_bad_arguments():
    from dinox import ops
    base = dict(pred=U8, labels=U8, spacing=SP, num_classes=3)
    cases = [
        (dict(pred=U8.float()), "pred must be uint8"), (dict(labels=U8.int()), "labels must be uint8"), (dict(pred=U8[0]), "pred must be uint8"),
        (dict(pred=U8[None]), "pred must be uint8"), (dict(labels=U8[:, :4]), "differ in shape"),
        (dict(pred=torch.zeros((1025, 1, 1), dtype=torch.uint8), labels=torch.zeros((1025, 1, 1), dtype=torch.uint8)), "1024"),
        (dict(pred=torch.zeros((1, 1025, 1), dtype=torch.uint8), labels=torch.zeros((1, 1025, 1), dtype=torch.uint8)), "1024"),
        (dict(pred=torch.zeros((1, 1, 1025), dtype=torch.uint8), labels=torch.zeros((1, 1, 1025), dtype=torch.uint8)), "1024"),
        (dict(pred=torch.zeros((0, 4, 4), dtype=torch.uint8), labels=torch.zeros((0, 4, 4), dtype=torch.uint8)), "1 <= Z"),
        (dict(num_classes=1), "num_classes"), (dict(num_classes=65), "num_classes"), (dict(num_classes=2.0), "num_classes"),
        (dict(num_classes=True), "num_classes"),
        (dict(tolerances=()), "tolerances"), (dict(tolerances=[1.0] * 9), "tolerances"), (dict(tolerances=(-1.0,)), "tolerances"),
        (dict(tolerances=(float("nan"),)), "tolerances"), (dict(tolerances=(float("inf"),)), "tolerances"), (dict(tolerances=1.0), "tolerances"),
        (dict(q=(0, 100)), "q must be"), (dict(q=(101, 100)), "q must be"), (dict(q=0.95), "q must be"), (dict(q=(95.0, 100)), "q must be"),
        (dict(q=(1, 2, 3)), "q must be"), (dict(q=(True, 1)), "q must be"),
        (dict(spacing=(1.0, 1.0)), "spacing"), (dict(spacing=(1.0, 1.0, 0.0)), "spacing"), (dict(spacing=(1.0, -1.0, 1.0)), "spacing"),
        (dict(spacing=(float("nan"), 1.0, 1.0)), "spacing"), (dict(spacing=(1.0, float("inf"), 1.0)), "spacing"), (dict(spacing=1.0), "spacing"),
        (dict(spacing=(1.0, 1.0, 1e-50)), "spacing"), (dict(spacing=torch.ones(2, 3)), "spacing"), (dict(spacing=("a", 1.0, 1.0)), "spacing"),
    ]
    for kw, msg in cases:
        args = dict(base)
        args.update(kw)
        with pytest.raises(ValueError, match=msg) as e:
            ops.surface_stats_3d(**args)
        assert str(e.value).startswith("surface_stats_3d:"), (kw, str(e.value))
    with pytest.raises(RuntimeError, match="CUDA/HIP device"):      # argument errors first, then: no CPU path
        ops.surface_stats_3d(**base)
    with pytest.raises(RuntimeError, match="CUDA/HIP device"):
        ops.surface_stats_3d(U8, U8, torch.tensor([2.5, 0.7, 1.3]), 3, tolerances=(1.0, 2.0), q=(1, 1))


# ------------------------------------------------------------------------------------------ dinox.segment.surface_metrics_3d
def test_surface_metrics_3d_on_fabricated_outputs():
    from dinox.segment import SurfaceAccumulator, surface_metrics_3d
    C, T = 5, 2
    counts = np.zeros((C, 2, 1 + T), np.int64)
    values = np.zeros((C, 2, 3), np.float32)
    counts[0] = [[40, 30, 36], [60, 45, 57]]
    values[0] = [[20.0, 3.0, 2.0], [45.0, 4.5, 2.5]]
    counts[1] = [[10, 10, 10], [10, 10, 10]]                  # a perfect class: zeros everywhere
    counts[2, 0, 0] = 7                                       # only in pred
    counts[3, 1, 0] = 9                                       # only in gt; class 4 in neither
    shape = (6, 40, 36)
    m = surface_metrics_3d(torch.from_numpy(counts), torch.from_numpy(values), SP, shape)
    assert set(m) == {"hd95", "hd", "assd", "nsd"} and all(v.dtype == torch.float64 and not v.is_cuda for v in m.values())
    assert tuple(m["hd95"].shape) == (1, C) and tuple(m["nsd"].shape) == (1, C, T)
    diag = math.sqrt((2.5 * 6) ** 2 + (0.7 * 40) ** 2 + (1.3 * 36) ** 2)
    assert m["hd95"][0].tolist()[:4] == pytest.approx([2.5, 0.0, diag, diag], rel=1e-15) and math.isnan(m["hd95"][0, 4])
    assert m["hd"][0].tolist()[:4] == pytest.approx([4.5, 0.0, diag, diag], rel=1e-15) and math.isnan(m["hd"][0, 4])
    assert m["assd"][0].tolist()[:4] == pytest.approx([0.65, 0.0, diag, diag], rel=1e-15) and math.isnan(m["assd"][0, 4])
    assert m["nsd"][0, :4].ravel().tolist() == pytest.approx([0.75, 0.93, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0], rel=1e-15)
    assert torch.isnan(m["nsd"][0, 4]).all()
    ref = SO.metrics(counts, values, SP, shape)               # the oracle's statement of the same rules
    for k in m:
        assert np.allclose(m[k].numpy(), ref[k], rtol=1e-15, atol=0, equal_nan=True), k
    acc = SurfaceAccumulator(C, T)                            # the layout the accumulator takes: one volume is one "image"
    acc.update(m)
    assert acc.result()["images"].tolist() == [1, 1, 1, 1, 0]
    for bad in ((counts[None], values[None]), (counts, values[:, :, :2]), (counts[:, :1], values[:, :1]), (counts[:, :, :1], values)):
        with pytest.raises(ValueError, match="surface_metrics_3d: counts must be"):
            surface_metrics_3d(torch.from_numpy(bad[0]), torch.from_numpy(bad[1]), SP, shape)
    for sp, shp in (((1.0, 1.0), shape), (SP, (40, 36))):
        with pytest.raises(ValueError, match="surface_metrics_3d: spacing must be"):
            surface_metrics_3d(torch.from_numpy(counts), torch.from_numpy(values), sp, shp)


def test_the_2d_metrics_are_what_they_were():
    """surface_metrics now shares its body with surface_metrics_3d: the same fabricated batch against the oracle of the 2-D path."""
    import _surface_oracle as SO2
    from dinox.segment import surface_metrics
    counts = np.zeros((2, 3, 2, 2), np.int64)
    values = np.zeros((2, 3, 2, 3), np.float32)
    counts[0, 0], values[0, 0] = [[40, 30], [60, 45]], [[20.0, 3.0, 2.0], [45.0, 4.5, 2.5]]
    counts[0, 1, 0, 0], counts[1, 2, 1, 0] = 7, 9
    sp = np.array([[0.7, 1.3], [2.5, 0.6]])
    m, ref = surface_metrics(counts, values, sp, (32, 48)), SO2.metrics(counts, values, sp, (32, 48))
    for k in ref:
        assert np.allclose(m[k].numpy(), ref[k], rtol=1e-15, atol=0, equal_nan=True), k


# ------------------------------------------------------------------------------------------ scripts/segment_volume.py
def _script():
    if "segment_volume" in sys.modules:
        return sys.modules["segment_volume"]
    spec = importlib.util.spec_from_file_location("segment_volume", os.path.join(ROOT, "dino-x_amd", "scripts", "segment_volume.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


BASE = ["--backbone", "b", "--segmenter", "s", "--volume", "v.npy", "--spacing", "0.8", "0.7", "2.5", "--out", "o.npy"]


def test_script_parser_takes_the_surface_flags():
    sv = _script()
    a = sv.build_parser().parse_args(BASE)
    assert a.tolerance_mm is None and a.surface_quantile == [95, 100]
    sv.check_args(sv.build_parser(), a)
    a = sv.build_parser().parse_args(BASE + ["--labels", "g.npy", "--tolerance-mm", "1", "--tolerance-mm", "2.5", "--surface-quantile", "1", "2",
                                             "--report", "r.json"])
    assert a.tolerance_mm == [1.0, 2.5] and a.surface_quantile == [1, 2]
    sv.check_args(sv.build_parser(), a)


def test_script_refuses_bad_surface_arguments(capsys):
    sv = _script()
    lab = ["--labels", "g.npy"]
    for extra, msg in ((["--tolerance-mm", "1"], "--tolerance-mm needs --labels"), (lab + ["--tolerance-mm", "-1"], "--tolerance-mm"),
                       (lab + ["--tolerance-mm", "nan"], "--tolerance-mm"), (lab + ["--tolerance-mm", "inf"], "--tolerance-mm"),
                       (lab + ["--tolerance-mm", "1"] * 9, "--tolerance-mm"), (["--surface-quantile", "0", "100"], "--surface-quantile"),
                       (["--surface-quantile", "3", "2"], "--surface-quantile")):
        with pytest.raises(SystemExit) as e:
            sv.run(sv.build_parser().parse_args(BASE + extra))
        assert msg in str(e.value.code) + capsys.readouterr().err, extra
    with pytest.raises(SystemExit):
        sv.build_parser().parse_args(BASE + ["--surface-quantile", "95"])
    assert "--surface-quantile" in capsys.readouterr().err
