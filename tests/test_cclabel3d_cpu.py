"""CPU checks of the whole-volume connected-component path: the oracle (tests/_cc3d_oracle.py) on hand-made volumes with known answers,
its two labellers against each other, the filter and the lesion counts on hand-made volumes, dinox.segment.min_component_vox /
resample_labels_nearest / CaseAccumulator on hand numbers, every argument refusal of ops.cc_label_3d / cc_filter_3d / lesion_counts_3d and of
the four C entries (host checks, nothing is launched), and the parser of scripts/segment_volume.py."""
import importlib.util
import math
import os
import sys

import numpy as np
import pytest
import torch

import _cc3d_oracle as O
from conftest import ROOT

LABELLERS = (O.label_flood, O.label_propagate)
CONNS = (6, 18, 26)


# ------------------------------------------------------------------------------------------ the oracle on volumes with known answers
@pytest.mark.parametrize("label", LABELLERS)
def test_two_voxels_sharing_only_a_corner(label):
    v = np.zeros((2, 2, 2), np.uint8)
    v[0, 0, 0] = v[1, 1, 1] = 1
    comp, area, ncomp = label(v, 2, 26)
    assert comp[1, 1, 1] == comp[0, 0, 0] == 0 and area[0, 0, 0] == 2 and ncomp[1] == 1
    for conn in (18, 6):
        comp, area, ncomp = label(v, 2, conn)
        assert comp[1, 1, 1] == 7 and area[0, 0, 0] == 1 and area[1, 1, 1] == 1 and ncomp[1] == 2
    assert comp.dtype == np.int32 and area.dtype == np.int32 and ncomp.dtype == np.int64


@pytest.mark.parametrize("label", LABELLERS)
def test_two_voxels_sharing_only_an_edge_across_z(label):
    v = np.zeros((2, 2, 2), np.uint8)
    v[0, 0, 0] = v[1, 0, 1] = 1                    # dz = 1, dx = 1
    for conn in (18, 26):
        comp, area, ncomp = label(v, 2, conn)
        assert comp[1, 0, 1] == 0 and area[0, 0, 0] == 2 and ncomp[1] == 1
    comp, area, ncomp = label(v, 2, 6)
    assert comp[1, 0, 1] == 5 and ncomp[1] == 2
    assert ncomp[0] == 1                           # the six background voxels stay one component through their faces


@pytest.mark.parametrize("label", LABELLERS)
def test_shell_with_a_hole(label):
    v = np.ones((3, 3, 3), np.uint8)
    v[1, 1, 1] = 0
    for conn in CONNS:
        comp, area, ncomp = label(v, 2, conn)
        assert area[0, 0, 0] == 26 and comp[1, 1, 1] == 13 and area[1, 1, 1] == 1 and ncomp.tolist() == [1, 1]
        assert (comp[v == 1] == 0).all() and area.sum() == 27


@pytest.mark.parametrize("label", LABELLERS)
def test_corner_meeting_where_four_tiles_meet_across_two_slices(label):
    v = np.zeros((2, 64, 64), np.uint8)
    v[0, 31, 31] = v[1, 32, 32] = 1                # one diagonal of the four-tile corner, one voxel per slice
    v[0, 31, 32] = v[1, 32, 31] = 2                # and the other
    comp, area, ncomp = label(v, 3, 26)
    assert comp[1, 32, 32] == comp[0, 31, 31] == 31 * 64 + 31 and area[0, 31, 31] == 2
    assert comp[1, 32, 31] == comp[0, 31, 32] == 31 * 64 + 32 and area[0, 31, 32] == 2
    assert ncomp.tolist() == [1, 1, 1]
    for conn in (18, 6):
        comp, area, ncomp = label(v, 3, conn)
        assert ncomp.tolist() == [1, 2, 2] and comp[1, 32, 32] == (64 + 32) * 64 + 32


def test_mask_and_values_outside_the_classes():
    v = np.array([[[1, 1, 1, 1]], [[0, 255, 1, 3]]], np.uint8)
    mask = np.array([[[0, 255, 0, 0]], [[0, 0, 0, 255]]], np.uint8)
    comp, area, ncomp = O.label_flood(v, 2, 6, mask)
    assert comp.tolist() == [[[0, -1, 2, 2]], [[4, -1, 2, -1]]] and ncomp.tolist() == [1, 2] and area[0, 0, 2] == 3
    assert O.bad_values(v, 2) == 1 and O.bad_values(v, 2, mask) == 0


@pytest.mark.parametrize("shape", ((1, 1, 1), (1, 9, 1), (3, 5, 7), (4, 33, 40)))
@pytest.mark.parametrize("conn", CONNS)
def test_the_two_labellers_agree(shape, conn):
    for vol in (O.structured(shape), O.noise(shape)):
        for mask in (None, O.mask_of(shape)):
            a, b = O.label_flood(vol, 3, conn, mask), O.label_propagate(vol, 3, conn, mask)
            for x, y in zip(a, b):
                assert x.dtype == y.dtype and np.array_equal(x, y)
            comp, area, ncomp = a
            assert area.sum() == (comp >= 0).sum() and (area > 0).sum() == ncomp.sum()


def test_structured_volumes_have_the_components_they_are_named_for():
    cb = O.checkerboard((6, 40, 40))
    assert O.label_propagate(cb, 2, 6)[2].tolist() == [4800, 4800]
    assert O.label_propagate(cb, 2, 18)[2].tolist() == [1, 1] and O.label_propagate(cb, 2, 26)[2].tolist() == [1, 1]
    sp = O.serpentine((6, 40, 40))
    for conn in CONNS:
        comp, area, ncomp = O.label_propagate(sp, 2, conn)
        assert ncomp[1] == 1 and area[0, 0, 0] == (sp == 1).sum() and (sp[1::2] == 1).sum() == 3


# ------------------------------------------------------------------------------------------ filter and lesion counts on hand-made volumes
def _blobs():
    v = np.zeros((3, 4, 6), np.uint8)
    v[0, 0, 0:2] = 1                               # A: 4 voxels over two slices, root 0
    v[1, 0, 0:2] = 1
    v[1:3, 3, 4:6] = 1                             # B: 4 voxels, root (1 * 4 + 3) * 6 + 4 = 46
    v[2, 0, 3] = 1                                 # D: 1 voxel
    v[0, 2, 2:5] = 2                               # E: 3 voxels of class 2
    return v


def test_filter_ties_and_the_minimum_exactly_at_the_boundary():
    v = _blobs()
    out = O.cc_filter(v, 3, keep_largest=True, connectivity=6)
    assert (out == 1).sum() == 4 and out[0, 0, 0] == 1 and out[1, 3, 4] == 0      # equal volumes: the lower root wins
    assert (out == 2).sum() == 3
    assert (O.cc_filter(v, 3, min_vox=4)[v == 1] == 1).sum() == 8                # area == min_vox is kept
    assert (O.cc_filter(v, 3, min_vox=5) == 1).sum() == 0 and (O.cc_filter(v, 3, min_vox=4) == 2).sum() == 0
    assert (O.cc_filter(v, 3, min_vox=3) == 2).sum() == 3
    assert np.array_equal(O.cc_filter(v, 3, min_vox=100, first_class=2) == 1, v == 1)   # classes below first_class are left alone
    assert np.array_equal(O.cc_filter(v, 3), v) and np.array_equal(O.cc_filter(v, 3, min_vox=0), v)
    # the largest is chosen among all components, whatever min_vox says
    assert (O.cc_filter(v, 3, min_vox=5, keep_largest=True) == 1).sum() == 0


def test_lesion_counts_on_a_hand_made_pair():
    gt = _blobs()
    pred = np.zeros_like(gt)
    pred[0, 0, 0:2] = 1                            # half of A (2 of its 4 voxels), and nothing of B
    pred[2, 0, 3] = 1                              # all of D
    pred[0, 3, 0] = 1                              # a false positive
    pred[0, 2, 2] = 2                              # a third of E
    assert O.lesion_counts(pred, gt, 3, 6, (0, 1)).tolist() == [[1, 1, 1, 1], [3, 2, 3, 2], [1, 1, 1, 1]]
    assert O.lesion_counts(pred, gt, 3, 6, (3, 4)).tolist() == [[1, 1, 1, 1], [3, 1, 3, 2], [1, 0, 1, 1]]
    assert O.lesion_counts(pred, gt, 3, 6, (0, 1), min_vox=2)[1].tolist() == [2, 1, 1, 1]
    gt2 = gt.copy()
    gt2[0, 3, 0] = 255                             # the false positive falls on an ignored voxel: it is no component any more
    assert O.lesion_counts(pred, gt2, 3, 6, (0, 1))[1].tolist() == [3, 2, 2, 2]


# ------------------------------------------------------------------------------------------ dinox.segment helpers on hand numbers
def test_min_component_vox():
    from dinox.segment import min_component_vox
    assert min_component_vox(0.0) == 0 and min_component_vox(10.0) == 10 and min_component_vox(10.5) == 11
    assert min_component_vox(10.0, (2.5, 0.5, 0.5)) == 16 and min_component_vox(10.1, (2.5, 0.5, 0.5)) == 17
    for v, sp in ((50.0, (2.5, 0.7, 0.8)), (1e-9, (1.0, 1.0, 1.0)), (3.0, (0.3, 0.1, 0.1))):
        assert min_component_vox(v, sp) == O.min_vox(v, sp)
    for kw in (dict(min_volume_mm3=-1.0), dict(min_volume_mm3=math.nan), dict(min_volume_mm3=math.inf), dict(voxel_mm=(1.0, 1.0)),
               dict(voxel_mm=(1.0, 0.0, 1.0)), dict(voxel_mm=(1.0, -1.0, 1.0)), dict(voxel_mm=(1.0, math.nan, 1.0)),
               dict(min_volume_mm3=1e30)):
        args = dict(min_volume_mm3=1.0, voxel_mm=(1.0, 1.0, 1.0))
        args.update(kw)
        with pytest.raises(ValueError):
            min_component_vox(**args)


def test_resample_labels_nearest():
    from dinox.segment import resample_labels_nearest
    rng = np.random.default_rng(0)
    lab = rng.integers(0, 4, size=(3, 8, 6)).astype(np.uint8)
    lab[0, 0, 0] = lab[2, 7, 5] = 255
    assert np.array_equal(resample_labels_nearest(lab[:, :6], 6), lab[:, :6])                    # identity at H = W = S
    out = resample_labels_nearest(np.ascontiguousarray(lab[:, :, :4]), 4)                        # H 8 -> 4 is 2:1, W 4 -> 4 is 1:1
    assert out.shape == (3, 4, 4) and np.array_equal(out, lab[:, 1::2, :4])                       # floor((i + 0.5) 2) = 2 i + 1
    up = resample_labels_nearest(lab, 12)                                                         # 2:3 and 1:2 upwards
    iy = [min(int(math.floor((i + 0.5) * 8 / 12)), 7) for i in range(12)]
    ix = [min(int(math.floor((j + 0.5) * 6 / 12)), 5) for j in range(12)]
    assert np.array_equal(up, lab[:, iy][:, :, ix]) and up[0, 0, 0] == 255 and up[2, 11, 11] == 255
    assert set(np.unique(up)) <= set(np.unique(lab)) and up.dtype == np.uint8 and up.flags["C_CONTIGUOUS"]
    for bad, S in ((lab[0], 4), (lab.astype(np.int32), 4), (lab, 0), (lab, 2.5)):
        with pytest.raises(ValueError, match="resample_labels_nearest"):
            resample_labels_nearest(bad, S)


def test_case_accumulator_on_hand_numbers():
    from dinox.segment import CaseAccumulator
    acc = CaseAccumulator(3)
    # case 1: class 1 Dice 2 * 3 / (4 + 6) = 0.6, class 2 absent from both maps
    acc.update(torch.tensor([[90, 3, 0], [92, 4, 0], [94, 6, 0]]), torch.tensor([[1, 1, 1, 1], [2, 1, 3, 1], [0, 0, 0, 0]]))
    # case 2: class 1 Dice 1.0, class 2 predicted but not labelled: Dice 0
    acc.update(torch.tensor([[50, 5, 0], [50, 5, 7], [57, 5, 0]]), torch.tensor([[1, 1, 1, 1], [1, 1, 1, 1], [0, 0, 2, 0]]))
    r = acc.result()
    assert r["cases"].tolist() == [2, 2, 1]
    assert r["dice"].tolist() == pytest.approx([(180 / 186 + 100 / 107) / 2, 0.8, 0.0])
    les = r["lesions"]
    assert les["images"] == 2 and les["n_gt"].tolist() == [2, 3, 0] and les["n_pred"].tolist() == [2, 4, 2]
    assert les["sensitivity"][1].item() == pytest.approx(2 / 3) and les["precision"][1].item() == 0.5
    assert les["fp_per_image"].tolist() == [0.0, 1.0, 1.0] and math.isnan(les["sensitivity"][2].item())
    assert math.isnan(CaseAccumulator(2).result()["dice"][0].item())
    for bad in ((torch.zeros((3, 2), dtype=torch.int64), torch.zeros((3, 4), dtype=torch.int64)),
                (torch.zeros((3, 3)), torch.zeros((3, 4), dtype=torch.int64)), (torch.zeros((3, 3), dtype=torch.int64), torch.zeros((4, 3), dtype=torch.int64))):
        with pytest.raises(ValueError, match="CaseAccumulator"):
            acc.update(*bad)


def test_volume_helpers_refuse_bad_arguments():
    from dinox.segment import postprocess_volume, segment_volume
    with pytest.raises(ValueError, match="postprocess_volume"):
        postprocess_volume(np.zeros((2, 4, 4), np.uint8), 3)
    with pytest.raises(ValueError, match="min_volume_mm3"):
        postprocess_volume(torch.zeros((2, 4, 4), dtype=torch.uint8), 3, min_volume_mm3=-1.0)
    with pytest.raises(RuntimeError, match="CUDA/HIP device"):
        postprocess_volume(torch.zeros((2, 4, 4), dtype=torch.uint8), 3, keep_largest=True)
    with pytest.raises(ValueError, match="min_volume_mm3"):
        segment_volume(None, np.zeros((2, 4, 4), np.float32), min_volume_mm3=-2.0)
    with pytest.raises(ValueError, match="connectivity"):
        segment_volume(None, np.zeros((2, 4, 4), np.float32), connectivity=8)


# ------------------------------------------------------------------------------------------ ops: refusals
U8 = torch.zeros((2, 8, 8), dtype=torch.uint8)
COMMON = [
    (dict(volume=U8.float()), "must be uint8"),
    (dict(volume=U8[0]), "must be uint8"),
    (dict(volume=U8[None]), "must be uint8"),
    (dict(volume=torch.zeros((1, 1025, 4), dtype=torch.uint8)), "1024"),
    (dict(volume=torch.zeros((1, 4, 1025), dtype=torch.uint8)), "1024"),
    (dict(volume=torch.zeros((0, 4, 4), dtype=torch.uint8)), "Z >= 1"),
    (dict(volume=torch.zeros(1, dtype=torch.uint8).expand(1025, 1024, 1024)), "2\\^30"),
    (dict(num_classes=1), "num_classes"),
    (dict(num_classes=65), "num_classes"),
    (dict(num_classes=2.0), "num_classes"),
    (dict(num_classes=True), "num_classes"),
    (dict(connectivity=4), "connectivity"),
    (dict(connectivity=8), "connectivity"),
    (dict(connectivity=27), "connectivity"),
    (dict(connectivity=26.0), "connectivity"),
]
MIN_VOX = [(dict(min_vox=1.5), "min_vox"), (dict(min_vox=-1), "min_vox"), (dict(min_vox=1 << 31), "min_vox"), (dict(min_vox=True), "min_vox"),
           (dict(min_vox=[1, 2]), "min_vox"), (dict(min_vox=torch.tensor(3)), "min_vox")]


def _refused(fn, name, base, cases):
    for kw, msg in cases:
        args = dict(base)
        args.update(kw)
        with pytest.raises(ValueError, match=msg) as e:
            fn(**args)
        assert name in str(e.value), (kw, str(e.value))
    with pytest.raises(RuntimeError, match="CUDA/HIP device"):      # argument errors first, then: no CPU path
        fn(**base)


def test_cc_label_3d_refuses_bad_arguments():
    from dinox import ops
    _refused(ops.cc_label_3d, "cc_label_3d", dict(volume=U8, num_classes=3), COMMON + [
        (dict(mask=U8.int()), "mask must be uint8"), (dict(mask=U8[:, :4]), "differ in shape")])


def test_cc_filter_3d_refuses_bad_arguments():
    from dinox import ops
    _refused(ops.cc_filter_3d, "cc_filter_3d", dict(volume=U8, num_classes=3), COMMON + MIN_VOX + [
        (dict(mask=U8[:1]), "differ in shape"), (dict(targets=U8.long()), "targets must be uint8"), (dict(targets=U8[:, :, :4]), "differ in shape"),
        (dict(first_class=-1), "first_class"), (dict(first_class=4), "first_class"), (dict(first_class=1.0), "first_class"),
        (dict(keep_largest="yes"), "keep_largest")])


def test_lesion_counts_3d_refuses_bad_arguments():
    from dinox import ops
    cases = [(dict(pred=kw["volume"], labels=kw["volume"]) if "volume" in kw else kw, msg) for kw, msg in COMMON]
    _refused(ops.lesion_counts_3d, "lesion_counts_3d", dict(pred=U8, labels=U8, num_classes=3), cases + MIN_VOX + [
        (dict(labels=U8.float()), "labels must be uint8"), (dict(labels=U8[:, :4]), "differ in shape"),
        (dict(overlap=0.5), "overlap"), (dict(overlap=(1, 0)), "overlap"), (dict(overlap=(2, 1)), "overlap"), (dict(overlap=(-1, 2)), "overlap"),
        (dict(overlap=(0.5, 1)), "overlap"), (dict(overlap=(1, 1 << 20)), "overlap"), (dict(overlap=(1, 2, 3)), "overlap")])


def test_c_entries_check_their_arguments_before_any_launch():
    from dinox import _lib
    lib = _lib.lib
    assert lib.dinox_cc3d_ws_bytes(3, 300, 70, 5) == 8 * 3 * 300 * 70 + 8 * 5
    assert lib.dinox_cc3d_ws_bytes(1024, 1024, 1024, 64) == 8 * (1 << 30) + 8 * 64
    assert lib.dinox_cc3d_ws_bytes(1 << 30, 1, 1, 2) > 0
    for sizes in ((0, 8, 8, 2), (1, 0, 8, 2), (1, 8, 1025, 2), (1, 1025, 8, 2), (1, 8, 8, 1), (1, 8, 8, 65), (1025, 1024, 1024, 2),
                  ((1 << 30) + 1, 1, 1, 2), (1 << 40, 1, 1, 2), (-1, 8, 8, 2)):
        assert lib.dinox_cc3d_ws_bytes(*sizes) == 0, sizes
    p = 0x1000                                     # never dereferenced: every call below is refused on the host
    sizes = [(dict(H=0), "H=0"), (dict(W=1025), "W=1025"), (dict(C=1), "C=1"), (dict(C=65), "C=65"), (dict(Z=0), "Z=0"),
             (dict(Z=1025, H=1024, W=1024), "Z=1025")]
    ok = dict(Z=2, H=8, W=8, C=2)

    def label(a, conn=26, labels=p, bad=p):
        return lib.dinox_cc3d_label(labels, None, p, p, p, bad, p, a["Z"], a["H"], a["W"], a["C"], conn, None)

    def filt(a, c0=1, y=None, counts=None, out=p, mv=1):
        return lib.dinox_cc3d_filter(p, p, p, mv, y, out, counts, p, a["Z"], a["H"], a["W"], a["C"], c0, 0, None)

    def match(a, tn=0, td=1, gt=p, mv=1):
        return lib.dinox_cc3d_match(p, p, p, gt, p, p, mv, p, p, a["Z"], a["H"], a["W"], a["C"], tn, td, None)

    for name, call in (("cc3d_label", label), ("cc3d_filter", filt), ("cc3d_match", match)):
        for kw, msg in sizes:
            assert call(dict(ok, **kw)) == -1 and msg in _lib.last_error() and name in _lib.last_error(), (name, kw, _lib.last_error())
    for conn in (0, 4, 8, 9, 27):
        assert label(ok, conn=conn) == -1 and f"connectivity={conn}" in _lib.last_error() and "cc3d_label" in _lib.last_error()
    assert label(ok, labels=None) == -1 and "null pointer" in _lib.last_error()
    assert label(ok, bad=None) == -1 and "null pointer" in _lib.last_error()
    assert filt(ok, out=None) == -1 and "null pointer" in _lib.last_error()
    assert filt(ok, y=p) == -1 and "both or neither" in _lib.last_error()
    assert filt(ok, counts=p) == -1 and "both or neither" in _lib.last_error()
    assert filt(ok, mv=-1) == -1 and "min_vox=-1" in _lib.last_error() and "cc3d_filter" in _lib.last_error()
    for c0 in (-1, 3):
        assert filt(ok, c0=c0) == -1 and f"c0={c0}" in _lib.last_error()
    assert match(ok, gt=None) == -1 and "null pointer" in _lib.last_error()
    assert match(ok, mv=-5) == -1 and "min_vox=-5" in _lib.last_error() and "cc3d_match" in _lib.last_error()
    for tn, td in ((-1, 2), (3, 2), (0, 0), (1, 1 << 20)):
        assert match(ok, tn=tn, td=td) == -1 and f"overlap {tn}/{td}" in _lib.last_error()


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


def test_script_parser_defaults():
    sv = _script()
    a = sv.build_parser().parse_args(BASE)
    assert [str(v) for v in a.volume] == ["v.npy"] and a.spacing == [0.8, 0.7, 2.5] and str(a.out) == "o.npy"
    assert (a.keep_largest, a.min_component_mm3, a.connectivity, a.labels, a.lesion_overlap, a.report) == (False, 0.0, 26, None, 0.0, None)
    assert (a.context, a.batch_size, a.no_amp, a.input_format) == ("neighbours", 64, False, "hu16_png")   # the fine-tuning scripts' default
    a = sv.build_parser().parse_args(BASE + ["--volume", "w.npy", "--labels", "g.npy", "--labels", "h.npy", "--connectivity", "6", "--keep-largest",
                                             "--min-component-mm3", "50", "--lesion-overlap", "0.25", "--report", "r.json", "--context", "replicate"])
    assert [str(v) for v in a.volume] == ["v.npy", "w.npy"] and [str(v) for v in a.labels] == ["g.npy", "h.npy"]
    assert (a.keep_largest, a.min_component_mm3, a.connectivity, a.lesion_overlap, str(a.report), a.context) == (True, 50.0, 6, 0.25, "r.json", "replicate")
    sv.check_args(sv.build_parser(), a)


def test_script_refuses_bad_arguments(capsys):
    sv = _script()
    for conn in ("8", "4", "9"):
        with pytest.raises(SystemExit):
            sv.build_parser().parse_args(BASE + ["--connectivity", conn])
        assert "--connectivity" in capsys.readouterr().err
    for extra, msg in ((["--min-component-mm3", "-1"], "--min-component-mm3"), (["--min-component-mm3", "nan"], "--min-component-mm3"),
                       (["--min-component-mm3", "inf"], "--min-component-mm3"), (["--lesion-overlap", "1.5"], "--lesion-overlap"),
                       (["--labels", "g.npy", "--labels", "h.npy"], "one per --volume"), (["--volume", "w.npy", "--labels", "g.npy"], "one per --volume"),
                       (["--report", "r.json"], "--report needs --labels"), (["--batch-size", "0"], "--batch-size")):
        with pytest.raises(SystemExit) as e:
            sv.run(sv.build_parser().parse_args(BASE + extra))
        assert msg in str(e.value.code) + capsys.readouterr().err, extra


def test_script_takes_labels_on_either_grid(tmp_path, capsys):
    sv = _script()
    ap = sv.build_parser()
    rng = np.random.default_rng(0)
    src = rng.integers(0, 3, size=(2, 12, 10)).astype(np.uint8)
    np.save(tmp_path / "src.npy", src)
    np.save(tmp_path / "grid.npy", src[:, :8, :8].copy())
    np.save(tmp_path / "odd.npy", src[:, :5])
    np.save(tmp_path / "i32.npy", src.astype(np.int32))
    from dinox.segment import resample_labels_nearest
    assert np.array_equal(sv.grid_labels(ap, tmp_path / "src.npy", (2, 12, 10), 8), resample_labels_nearest(src, 8))
    assert np.array_equal(sv.grid_labels(ap, tmp_path / "grid.npy", (2, 12, 10), 8), src[:, :8, :8])
    for name in ("odd.npy", "i32.npy"):
        with pytest.raises(SystemExit):
            sv.grid_labels(ap, tmp_path / name, (2, 12, 10), 8)
        assert "--labels" in capsys.readouterr().err
