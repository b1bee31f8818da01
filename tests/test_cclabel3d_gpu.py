"""GPU tests of the whole-volume connected-component path: csrc/cclabel3d.hip (on the stages of csrc/cclabel.hip) through ops.cc_label_3d /
cc_filter_3d / lesion_counts_3d, dinox.segment.postprocess_volume and segment_volume, bit for bit against tests/_cc3d_oracle.py.  The
shapes are the smallest that reach each seam: one voxel, one column, less than a tile, a partial second tile in both directions, the
four-tile corner across two slices, several tiles with ignored voxels."""
from functools import lru_cache

import numpy as np
import pytest
import torch

import _cc3d_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CONNS = (6, 18, 26)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _corner():
    v = np.zeros((4, 64, 64), np.uint8)
    v[1, 31, 31] = v[2, 32, 32] = 1                # one diagonal of the four-tile corner, in adjacent slices
    v[1, 31, 32] = v[2, 32, 31] = 2                # the other diagonal
    v[0, 10:50, 31:33] = 1                         # and a bar across the tile edge above them
    return v


def _slabs():
    v = np.zeros((6, 40, 40), np.uint8)
    v[0:3, 0:32, 0:32] = 1                         # a slab that fills the first tile of slices 0-2
    v[3:6, 32:40, 32:40] = 1                       # a slab in the last tile of slices 3-5
    v[3, 31, 31] = 1                               # ONE z link, on the tile corner: below (2, 31, 31), diagonal to (3, 32, 32) across four tiles
    return v


@lru_cache(maxsize=None)
def _volume(name):
    shapes = {"one": (1, 1, 1), "two": (2, 1, 1), "small": (3, 5, 7), "partial": (5, 33, 40), "noise": (9, 70, 33), "plane": (1, 70, 33)}
    if name in ("one", "two"):
        return np.ones(shapes[name], np.uint8)
    if name == "small":
        return O.noise(shapes[name], ignore=0.0, seed=3)
    if name == "partial":
        return O.structured(shapes[name], seed=4)
    if name in ("noise", "plane"):
        return O.noise(shapes[name], seed=5)
    return {"corner": _corner, "slabs": _slabs, "checker": lambda: O.checkerboard((6, 40, 40)), "serpentine": lambda: O.serpentine((6, 40, 40))}[name]()


@lru_cache(maxsize=None)
def _mask(name):
    return O.mask_of(_volume(name).shape, seed=7)


@lru_cache(maxsize=None)
def _want(name, conn, masked):
    """The oracle's labelling: computed once per case and shared, never changed."""
    return O.label_flood(_volume(name), 3, conn, _mask(name) if masked else None)


def _equal(got, want, what):
    for g, w, part in zip(got, want, ("comp", "area", "ncomp")):
        w = torch.from_numpy(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, part, g.dtype, tuple(g.shape))
        assert torch.equal(g.cpu(), w), (what, part, int((g.cpu() != w).sum()))


# ------------------------------------------------------------------------------------------ labelling
@pytest.mark.parametrize("name", ("one", "two", "small", "partial", "corner", "noise"))
@pytest.mark.parametrize("conn", CONNS)
def test_labelling_equals_the_oracle(name, conn):
    from dinox import ops
    vol = _dev(_volume(name))
    _equal(ops.cc_label_3d(vol, 3, conn), _want(name, conn, False), (name, conn))
    _equal(ops.cc_label_3d(vol, 3, conn, mask=_dev(_mask(name))), _want(name, conn, True), (name, conn, "mask"))


@pytest.mark.parametrize("conn", CONNS)
def test_structured_volumes(conn):
    from dinox import ops
    comp, area, ncomp = ops.cc_label_3d(_dev(_volume("checker")), 3, conn)
    _equal((comp, area, ncomp), _want("checker", conn, False), ("checker", conn))
    assert ncomp.tolist() == ([4800, 4800, 0] if conn == 6 else [1, 1, 0])
    sp = _volume("serpentine")
    comp, area, ncomp = ops.cc_label_3d(_dev(sp), 3, conn)
    _equal((comp, area, ncomp), _want("serpentine", conn, False), ("serpentine", conn))
    assert ncomp[1] == 1 and area[0, 0, 0] == int((sp == 1).sum())      # one path through every slice
    comp, area, ncomp = ops.cc_label_3d(_dev(_volume("slabs")), 3, conn)
    _equal((comp, area, ncomp), _want("slabs", conn, False), ("slabs", conn))
    assert ncomp[1] == (2 if conn == 6 else 1)     # the link voxel hangs below the first slab; only a corner joins it to the second


def test_one_slice_equals_the_image_kernel_and_two_calls_give_the_same_bits():
    from dinox import ops
    v = _dev(_volume("plane"))
    m = _dev(_mask("plane"))
    for conn3, conn2 in ((6, 4), (18, 8), (26, 8)):
        for mask in (None, m):
            got, ref = ops.cc_label_3d(v, 3, conn3, mask=mask), ops.cc_label(v, 3, conn2, mask=mask)
            assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]) and torch.equal(got[2], ref[2][0])
    big = _dev(_volume("noise"))
    a, b = ops.cc_label_3d(big, 3, 26), ops.cc_label_3d(big, 3, 26)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------ filter and lesion counts
def _ties():
    v = np.zeros((5, 36, 36), np.uint8)
    v[0:2, 0:2, 0:2] = 1                           # 8 voxels, root 0
    v[3:5, 30:32, 31:33] = 1                       # 8 voxels across the tile edge: the tie
    v[2, 20, 20:23] = 1                            # 3 voxels
    v[1:4, 10, 34] = 2                             # 3 voxels of class 2
    v[4, 35, 35] = 2
    return v


def test_filter_equals_the_oracle():
    from dinox import ops
    v = _ties()
    d = _dev(v)
    out = ops.cc_filter_3d(d, 3, keep_largest=True)
    assert torch.equal(out.cpu(), torch.from_numpy(O.cc_filter(v, 3, keep_largest=True)))
    assert int((out == 1).sum()) == 8 and out[0, 0, 0] == 1 and out[3, 30, 31] == 0          # equal volumes: the lower root wins
    for kw in (dict(min_vox=3), dict(min_vox=4), dict(min_vox=8), dict(min_vox=9), dict(min_vox=0), dict(min_vox=4, first_class=2),
               dict(min_vox=9, keep_largest=True), dict(keep_largest=True, connectivity=6, first_class=0)):
        assert torch.equal(ops.cc_filter_3d(d, 3, **kw).cpu(), torch.from_numpy(O.cc_filter(v, 3, **kw))), kw
    noise, gt = _volume("noise"), O.noise((9, 70, 33), seed=8)
    for kw in (dict(keep_largest=True), dict(min_vox=5, connectivity=6), dict(min_vox=40, connectivity=18, first_class=2)):
        want = O.cc_filter(noise, 3, mask=gt, **kw)
        out, counts = ops.cc_filter_3d(_dev(noise), 3, mask=_dev(gt), targets=_dev(gt), **kw)
        assert torch.equal(out.cpu(), torch.from_numpy(want)), kw
        wc, wbad = O.overlap_counts(want, gt, 3)
        assert wbad == 0 and counts.dtype == torch.int64 and torch.equal(counts.cpu(), torch.from_numpy(wc)), kw


@pytest.mark.parametrize("overlap", ((0, 1), (1, 2), (1, 1)))
def test_lesion_counts_equal_the_oracle(overlap):
    from dinox import ops
    gt = O.structured((5, 33, 40), seed=9)
    gt[O.mask_of(gt.shape, seed=10) == 255] = 255
    pred = O.structured((5, 33, 40), seed=11)
    for mv in (0, 3):
        got = ops.lesion_counts_3d(_dev(pred), _dev(gt), 3, connectivity=26, overlap=overlap, min_vox=mv)
        want = O.lesion_counts(pred, gt, 3, 26, overlap, min_vox=mv)
        assert got.dtype == torch.int64 and tuple(got.shape) == (3, 4) and torch.equal(got.cpu(), torch.from_numpy(want)), (overlap, mv)
    got = ops.lesion_counts_3d(_dev(pred), _dev(gt), 3, connectivity=6, overlap=overlap)
    assert torch.equal(got.cpu(), torch.from_numpy(O.lesion_counts(pred, gt, 3, 6, overlap)))


def test_a_label_outside_the_classes_is_refused():
    from dinox import ops
    v = _volume("small").copy()
    ok = _dev(v)
    v[2, 4, 6] = 3
    bad = _dev(v)
    with pytest.raises(ValueError, match="cc_label_3d: 1 value"):
        ops.cc_label_3d(bad, 3)
    with pytest.raises(ValueError, match="cc_filter_3d: 1 value"):
        ops.cc_filter_3d(bad, 3, keep_largest=True)
    with pytest.raises(ValueError, match="cc_filter_3d"):
        ops.cc_filter_3d(ok, 3, targets=bad)
    with pytest.raises(ValueError, match="lesion_counts_3d: 1 value\\(s\\) of pred"):
        ops.lesion_counts_3d(bad, ok, 3)
    with pytest.raises(ValueError, match="lesion_counts_3d: 1 value\\(s\\) of labels"):
        ops.lesion_counts_3d(ok, bad, 3)
    v[2, 4, 6] = 255                               # 255 is simply in no component
    assert int(ops.cc_label_3d(_dev(v), 3)[0][2, 4, 6]) == -1


# ------------------------------------------------------------------------------------------ segment_volume
TINY = dict(img_size=32, patch=8, dim=32, depth=2, heads=2, scale_aware=True)      # the configuration tests/test_segloss_gpu.py builds
SP = (0.8, 0.7, 2.5)


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


def test_segment_volume(seg_model):
    from dinox import ops
    from dinox.segment import postprocess_volume, segment_volume
    from zoo.encode import encode_volume
    vol = np.random.default_rng(11).integers(-400, 500, size=(5, 24, 30)).astype(np.int16)
    kw = dict(input_format="hu_float", hu_level=40.0, hu_width=400.0)
    got = segment_volume(seg_model, vol, SP, **kw)
    assert got.dtype == np.uint8 and got.shape == (5, 32, 32) and len(np.unique(got)) > 1
    assert np.array_equal(segment_volume(seg_model, vol, SP, batch_size=2, **kw), got)
    tokens = encode_volume(seg_model.backbone, vol, SP, return_all_tokens=True, **kw)
    with torch.no_grad():
        want = ops.seg_predict(seg_model.head(tokens, 16), 8)
    assert np.array_equal(got, want.cpu().numpy())
    clean = segment_volume(seg_model, vol, SP, keep_largest=True, min_volume_mm3=30.0, connectivity=18, **kw)
    voxel = (SP[2], SP[1] * 24 / 32, SP[0] * 30 / 32)
    ref = postprocess_volume(_dev(got), 3, voxel, keep_largest=True, min_volume_mm3=30.0, connectivity=18)
    assert np.array_equal(clean, ref.cpu().numpy())
    assert np.array_equal(clean, O.cc_filter(got, 3, min_vox=O.min_vox(30.0, voxel), keep_largest=True, connectivity=18))
