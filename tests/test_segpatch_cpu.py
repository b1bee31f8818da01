"""CPU tests of patch-based training at native resolution: the float64 oracle and the fp32 emulation of tests/_segpatch_oracle.py on exact
cases, against torch's grid_sample and on the GPU tests' own launches with five planted defects; the host refusals of
ops.seg_patch_sample before the library is touched; dinox.patches (PatchPool, patch_matrix, draw_patch_jobs); the command line.

Share of a job's pixels in the label band (an integer within delta of a coordinate) over the launches of tests/_segpatch_cases.py, from the
oracle alone: 0 in eight of the nine launches, 0.0002 in launch 8 (S = 70, one pixel of a job's 4900); the cap is 0.01."""
import importlib.util
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _segpatch_cases as K
import _segpatch_oracle as O
from conftest import ROOT
from dinox import patches as PT                              # the module and the op under test: nothing here runs without them
from dinox.ops import seg_patch_sample  # noqa: F401


def _plane(H, W, seed, classes=4):
    rng = np.random.default_rng(seed)
    return rng.random((H, W), dtype=np.float32), rng.integers(0, classes, size=(H, W)).astype(np.uint8)


def _both(planes, plane_of, par, S, mean=(0, 0, 0), std=(1, 1, 1), pad=0.0):
    want = O.sample64(planes, plane_of, par, S, mean, std, pad)
    x, m = O.emulate32(planes, plane_of, par, S, mean, std, pad)
    return want, x, m


# ------------------------------------------------------------------------------------------ exact cases
@pytest.mark.parametrize("S", [16, 27])
def test_exact_cases_to_the_bit(S):
    img, msk = _plane(S, S, S)
    ti, tm = torch.from_numpy(img), torch.from_numpy(msk)
    h = S / 2
    ident = tuple(float(v) for v in PT.patch_matrix((S // 2, S // 2), S, S).reshape(-1))     # T = S, centred: the identity, (1, 0, h, 0, 1, h)
    assert ident == (1, 0, h, 0, 1, h)
    jobs = {"identity": (ident, ti, tm), "mirror_x": ((-1, 0, h, 0, 1, h), ti.flip(-1), tm.flip(-1)),
            "mirror_y": ((1, 0, h, 0, -1, h), ti.flip(-2), tm.flip(-2))}
    # quarter turns: out[oy][ox] = in[sy][sx] with (sx, sy) = R (dx, dy) + (h, h); R = [[0, -1], [1, 0]] is torch.rot90 with k = 1
    for q, R in ((0, (1, 0, 0, 1)), (1, (0, -1, 1, 0)), (2, (-1, 0, 0, -1)), (3, (0, 1, -1, 0))):
        jobs[f"turn{q}"] = ((R[0], R[1], h, R[2], R[3], h), torch.rot90(ti, q, (0, 1)), torch.rot90(tm, q, (0, 1)))
    names = list(jobs)
    par = np.array([[*jobs[n][0], 1, 1] for n in names], dtype=np.float32)
    want, x, m = _both([(img, msk)], [0] * len(names), par, S)
    mean, std = np.float32(K.MEAN), np.float32(K.STD)
    xn, _ = O.emulate32([(img, msk)], [0] * len(names), par, S, mean, std, 0.0)
    for b, n in enumerate(names):
        ref_i, ref_m = jobs[n][1].numpy(), jobs[n][2].numpy()
        assert np.array_equal(want.m[b], ref_m) and np.array_equal(m[b], ref_m), n
        assert not want.band[b].any(), n
        for c in range(3):
            assert np.array_equal(want.x[b, c], ref_i.astype(np.float64)), n                 # the oracle: the plane's own values
            assert np.array_equal(x[b, c], ref_i), n                                           # the emulation: the same float32 bits
            assert np.array_equal(xn[b, c], (ref_i - mean[c]) / std[c]), n                     # and torch's normalisation, to the bit


def test_integer_translations_to_the_bit():
    S, H, W = 12, 20, 31
    img, msk = _plane(H, W, 5)
    shifts = [(0, 0), (3, 5), (-4, 2), (19, -7), (8, 19)]                                      # (ty, tx): out[oy][ox] = in[oy + ty][ox + tx]
    par = np.array([[1, 0, S / 2 + tx, 0, 1, S / 2 + ty, 1, 1] for ty, tx in shifts], dtype=np.float32)
    want, x, m = _both([(img, msk)], [0] * len(shifts), par, S, pad=0.25)
    big_i, big_m = np.full((H + 60, W + 60), np.float32(0.25)), np.full((H + 60, W + 60), 255, np.uint8)
    big_i[30:30 + H, 30:30 + W], big_m[30:30 + H, 30:30 + W] = img, msk
    for b, (ty, tx) in enumerate(shifts):
        ri, rm = big_i[30 + ty:30 + ty + S, 30 + tx:30 + tx + S], big_m[30 + ty:30 + ty + S, 30 + tx:30 + tx + S]
        assert np.array_equal(want.m[b], rm) and np.array_equal(m[b], rm)
        assert np.array_equal(want.x[b, 0], ri.astype(np.float64)) and np.array_equal(x[b, 1], ri)


# ------------------------------------------------------------------------------------------ against torch
def test_random_affines_agree_with_grid_sample():
    S, H, W = 23, 33, 41
    img, msk = _plane(H, W, 9)
    rng = np.random.default_rng(10)
    par = np.stack([K.job_par("affine0", H, W, S, rng) for _ in range(6)])
    want, x, m = _both([(img, msk)], [0] * 6, par, S)
    d = np.arange(S) + 0.5 - S / 2
    for b in range(6):
        a = par[b].astype(np.float64)
        sx = a[0] * d[None, :] + (a[1] * d[:, None] + a[2])
        sy = a[3] * d[None, :] + (a[4] * d[:, None] + a[5])
        grid = torch.from_numpy(np.stack([2 * sx / W - 1, 2 * sy / H - 1], -1))[None]
        ref = F.grid_sample(torch.from_numpy(img.astype(np.float64))[None, None], grid, mode="bilinear", padding_mode="zeros", align_corners=False)[0, 0]
        err = np.abs(ref.numpy() - want.x[b, 0])
        assert (err <= 1e-12).all(), err.max()                                                 # two float64 statements of one definition
        assert (np.abs(x[b, 0].astype(np.float64) - ref.numpy()) <= want.ex[b, 0] + 1e-12).all()   # the emulation inside the derived bound
        near = F.grid_sample(torch.from_numpy(msk.astype(np.float64))[None, None], grid, mode="nearest", padding_mode="zeros", align_corners=False)[0, 0]
        inside = (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
        ties = (np.abs(sx - np.rint(sx)) < 1e-6) | (np.abs(sy - np.rint(sy)) < 1e-6)
        keep = inside & ~ties
        assert keep.mean() > 0.3 and np.array_equal(near.numpy()[keep].astype(np.uint8), want.m[b][keep])
        assert (want.m[b][~inside] == 255).all()


# ------------------------------------------------------------------------------------------ the GPU launches, on the CPU
def _emulated(i, defect=None):
    c = K.launch(i)
    return O.emulate32(K.pool()[0], c["plane_of"], c["par"], c["S"], K.MEAN, K.STD, c["pad"], defect=defect)


def test_emulation_passes_every_gpu_launch_and_the_band_stays_under_the_cap():
    worst_share, worst_ratio = 0.0, 0.0
    for i in range(len(K.LAUNCHES)):
        x, m = _emulated(i)
        ratio, share = K.launch(i)["want"].check(x, m, m)
        worst_share, worst_ratio = max(worst_share, share), max(worst_ratio, ratio)
    print(f"largest band share {worst_share:.4f}, largest error / bound {worst_ratio:.3f}")
    assert worst_share <= 0.01
    kinds = {k for i in range(len(K.LAUNCHES)) for k in K.launch(i)["kinds"]}
    assert kinds == set(K.KINDS)


def test_far_and_zero_jobs():
    for i in range(len(K.LAUNCHES)):
        c = K.launch(i)
        for b, kind in enumerate(c["kinds"]):
            if kind == "far":
                assert (c["want"].m[b] == 255).all()
                for ch in range(3):
                    assert np.array_equal(c["want"].x[b, ch], np.full((c["S"], c["S"]), (np.float64(np.float32(c["pad"])) - np.float32(K.MEAN[ch]).astype(np.float64))
                                                              / np.float32(K.STD[ch]).astype(np.float64)))
            if kind == "zero":
                assert len(np.unique(c["want"].m[b])) == 1 and len(np.unique(c["want"].x[b, 0])) == 1


@pytest.mark.parametrize("defect", O.DEFECTS)
def test_planted_defect_is_caught(defect):
    caught = []
    for i in range(len(K.LAUNCHES)):
        x, m = _emulated(i, defect)
        try:
            K.launch(i)["want"].check(x, m)
        except AssertionError:
            caught.append(i)
    print(f"{defect}: caught in launches {caught}")
    assert caught, f"the planted defect {defect!r} passes every launch"


# ------------------------------------------------------------------------------------------ ops.seg_patch_sample: refusals on the host
class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"the library was touched: {name}")


def test_host_refusals(monkeypatch):
    from dinox import ops
    monkeypatch.setattr(ops, "lib", _Untouchable())
    img, msk = torch.zeros(100), torch.zeros(90, dtype=torch.uint8)
    ok = dict(img_pool=img, msk_pool=msk, jobs=[[10, 0, 9, 10]], par=[[1, 0, 0, 0, 1, 0, 1, 1]], S=8, mean=K.MEAN, std=K.STD)
    nan, inf = float("nan"), float("inf")
    for kw, msg in (
            (dict(jobs=[[11, 0, 9, 10]]), "leaves img_pool"), (dict(jobs=[[10, 1, 9, 10]]), "leaves msk_pool"), (dict(jobs=[[-1, 0, 9, 10]]), "leaves img_pool"),
            (dict(jobs=[[10, 0, 0, 10]]), r"must lie in \[1, 2\^20\]"), (dict(jobs=[[10, 0, 9, 0]]), r"must lie in \[1, 2\^20\]"),
            (dict(jobs=[[10, 0, 9, 1 << 21]]), r"must lie in \[1, 2\^20\]"), (dict(jobs=[[10, 0, 1 << 20, 1 << 20]]), "leaves img_pool"),
            (dict(par=[[nan, 0, 0, 0, 1, 0, 1, 1]]), "non-finite"), (dict(par=[[1, 0, inf, 0, 1, 0, 1, 1]]), "non-finite"),
            (dict(par=[[1, 0, 0, 0, 1, 0, 1, nan]]), "non-finite"), (dict(par=[[1, 0, 0, 0, 1, 0, 0, 1]]), "gamma"),
            (dict(par=[[1, 0, 0, 0, 1, 0, -1.5, 1]]), "gamma"), (dict(S=0), "S must be"), (dict(S=(1 << 14) + 1), "S must be"), (dict(S=True), "S must be"),
            (dict(jobs=np.zeros((0, 4), np.int64), par=np.zeros((0, 8), np.float32)), "what one grid takes"),
            (dict(jobs=[[10, 0, 9, 10]] * 600, par=[[1, 0, 0, 0, 1, 0, 1, 1]] * 600, S=1 << 14), "what one grid takes"),
            (dict(par=[[1, 0, 0, 0, 1, 0, 1, 1]] * 2), "rows of par"), (dict(jobs=[[10, 0, 9]]), "jobs must be"), (dict(jobs=[[10.0, 0, 9, 10]]), "jobs must be"),
            (dict(std=(0.2, 0.0, 0.2)), "std > 0"), (dict(mean=(0.2, nan, 0.2)), "std > 0"), (dict(pad=inf), "pad"),
            (dict(img_pool=img.double()), "img_pool must be"), (dict(msk_pool=msk.float()), "msk_pool must be"), (dict(img_pool=img.view(10, 10)), "img_pool must be"),
            (dict(out=(torch.zeros(1, 3, 8, 8), torch.zeros(1, 8, 9, dtype=torch.uint8))), "out must be")):
        with pytest.raises(ValueError, match=f"seg_patch_sample: .*{msg}"):
            ops.seg_patch_sample(**dict(ok, **kw))
    with pytest.raises(RuntimeError, match="CUDA/HIP device"):                                 # all checks passed: the device is asked for next
        ops.seg_patch_sample(**ok)


def test_c_entry_refuses_before_any_launch():
    import ctypes
    from dinox import _lib
    buf = (ctypes.c_float * 8)(0.5, 0.5, 0.5, 0.2, 0.2, 0.2, 0, 0)
    p, mean, std = ctypes.addressof(buf), ctypes.addressof(buf), ctypes.addressof(buf) + 12

    def call(**kw):
        a = dict(img=p, msk=p, jobs=p, par=p, x=p, m=p, B=1, S=8, mean=mean, std=std, pad=0.0)
        a.update(kw)
        return _lib.lib.dinox_seg_patch_sample(a["img"], a["msk"], a["jobs"], a["par"], a["x"], a["m"], a["B"], a["S"], a["mean"], a["std"], a["pad"], None)

    for name in ("img", "msk", "jobs", "par", "x", "m", "mean", "std"):
        assert call(**{name: None}) == -1 and "seg_patch_sample: null pointer" in _lib.last_error(), name
    for kw, msg in ((dict(S=0), "S=0"), (dict(S=(1 << 14) + 1), "S="), (dict(B=0), "B=0"), (dict(B=1 << 19, S=1 << 12), "runs"),
                    (dict(std=ctypes.addressof(buf) + 24), "std > 0"), (dict(pad=float("nan")), "pad=")):
        assert call(**kw) == -1 and msg in _lib.last_error(), (kw, _lib.last_error())


# ------------------------------------------------------------------------------------------ dinox.patches
def _pool(seed=0, **kw):
    from dinox.patches import PatchPool
    rng = np.random.default_rng(seed)
    imgs, msks = [], []
    for i, (H, W) in enumerate(((40, 52), (31, 47), (64, 64), (20, 20))):
        m = np.zeros((H, W), np.uint8)
        if i < 3:
            m[5:15, 8:20], m[18:26, 30:40] = 1, 2 + i % 2
            m[:, :2] = 255
        imgs.append(rng.random((H, W), dtype=np.float32))
        msks.append(m)
    return PatchPool(imgs, msks, [(0.5 + 0.1 * i, 0.7, 2.0) for i in range(4)], device="cpu", **kw), imgs, msks


def test_patch_pool():
    from dinox.patches import MAX_LOCATIONS, PatchPool
    pool, imgs, msks = _pool()
    assert len(pool) == 4 and pool.img.dtype == torch.float32 and pool.msk.dtype == torch.uint8
    assert pool.offsets.tolist() == [0, 40 * 52, 40 * 52 + 31 * 47, 40 * 52 + 31 * 47 + 64 * 64] and pool.img.numel() == pool.msk.numel() == pool.offsets[-1] + 400
    for i in range(4):
        o, (H, W) = int(pool.offsets[i]), pool.sizes[i]
        assert np.array_equal(pool.img[o:o + H * W].numpy().reshape(H, W), imgs[i]) and np.array_equal(pool.msk[o:o + H * W].numpy().reshape(H, W), msks[i])
        assert 255 not in pool.locations[i]
        for c, loc in pool.locations[i].items():
            assert (msks[i].reshape(-1)[loc] == c).all() and len(loc) == min((msks[i] == c).sum(), MAX_LOCATIONS)
    assert pool.foreground_classes(0) == [1, 2] and pool.foreground_classes(1) == [1, 3] and pool.foreground_classes(3) == [0]
    big = np.zeros((100, 100), np.uint8)
    capped = PatchPool([big.astype(np.float32)], [big], device="cpu", seed=3)
    again = PatchPool([big.astype(np.float32)], [big], device="cpu", seed=3)
    assert len(capped.locations[0][0]) == MAX_LOCATIONS and np.array_equal(capped.locations[0][0], again.locations[0][0])
    with pytest.raises(ValueError, match=r"need 0\.00 GiB on the device, above max_gib = 1e-09"):
        _pool(max_gib=1e-9)
    with pytest.raises(ValueError, match="must be equal"):
        PatchPool([big.astype(np.float32)], [big[:50]], device="cpu")


def test_patch_matrix_round_trips_the_centre():
    from dinox.patches import patch_matrix
    for S, t, cy, cx in ((16, 16, 7, 9), (27, 40, 100, 3), (224, 224, 511, 0), (15, 8, 0, 0)):
        for scale, ang, mx, my in ((1.0, 0.0, False, False), (1.3, 0.4, True, False), (0.6, -2.0, False, True), (2.0, math.pi / 2, True, True)):
            A = patch_matrix((cy, cx), t, S, scale, ang, mx, my)
            assert A.dtype == np.float32 and A.shape == (2, 3)
            sx, sy = O.coords32(np.array([*A.reshape(-1), 1, 1], np.float32), S)
            assert abs(float(sx[S // 2, S // 2]) - (cx + 0.5)) < 1e-3 and abs(float(sy[S // 2, S // 2]) - (cy + 0.5)) < 1e-3
            col0, col1 = math.hypot(A[0, 0], A[1, 0]), math.hypot(A[0, 1], A[1, 1])
            assert col0 == pytest.approx(scale * t / S, rel=1e-6) and col1 == pytest.approx(scale * t / S, rel=1e-6)
            assert (A[0, 0] * A[1, 1] - A[0, 1] * A[1, 0] < 0) == (mx != my)
    A = patch_matrix((5, 6), 32, 16)                       # scale 1, no angle, no mirror: one output pixel is t / S source pixels, axes apart
    assert A[0, 0] == 2 and A[1, 1] == 2 and A[0, 1] == 0 and A[1, 0] == 0


DRAW = dict(S=16, t=16, fg_prob=0.33, rotate_deg=15, scale_range=(0.7, 1.4))


def test_draw_patch_jobs_is_seeded_and_foreground_centred():
    from dinox.patches import draw_patch_jobs
    pool, imgs, msks = _pool()
    a = draw_patch_jobs(pool, 64, torch.Generator().manual_seed(5), **DRAW)
    b = draw_patch_jobs(pool, 64, torch.Generator().manual_seed(5), **DRAW)
    c = draw_patch_jobs(pool, 64, torch.Generator().manual_seed(6), **DRAW)
    assert all(np.array_equal(a[k], b[k]) for k in a) and not np.array_equal(a["par"], c["par"])
    assert a["jobs"].dtype == np.int64 and a["jobs"].shape == (64, 4) and a["par"].dtype == np.float32 and a["par"].shape == (64, 8)
    assert a["grid_spacing"].shape == (64, 2) and a["model_spacing"].shape == (64, 3) and set(a["sample"].tolist()) == {0, 1, 2, 3}
    assert (a["par"][:, 6] > 0).all() and np.isfinite(a["par"]).all()
    # unmirrored, unrotated, every job foreground-centred: the label at output pixel (S // 2, S // 2) is the chosen class
    for S in (16, 15):
        kw = dict(DRAW, S=S, t=24, fg_prob=1.0, rotate_deg=0.0, mirror=False)
        d = draw_patch_jobs(pool, 200, torch.Generator().manual_seed(7), **kw)
        planes = list(zip(imgs, msks))
        _, m = O.emulate32(planes, d["sample"].tolist(), d["par"], S, (0, 0, 0), (1, 1, 1), 0.0)
        want = O.sample64(planes, d["sample"].tolist(), d["par"], S, (0, 0, 0), (1, 1, 1), 0.0)
        assert (d["fg_class"] >= 0).all()
        assert np.array_equal(m[:, S // 2, S // 2], d["fg_class"]) and np.array_equal(want.m[:, S // 2, S // 2], d["fg_class"])
        for i in range(4):
            assert set(d["fg_class"][d["sample"] == i].tolist()) == set(pool.foreground_classes(i))   # background only where nothing else is
        # spacing: scale s on a sample of spacing (sx, sy, sz): the grid is (sy, sx) s t / S, the model hears (sx s, sy s, sz)
        s = np.hypot(d["par"][:, 0], d["par"][:, 3]) * S / 24
        sp = pool.spacings[d["sample"]]
        assert np.allclose(d["grid_spacing"], np.stack([sp[:, 1], sp[:, 0]], 1) * (s * 24 / S)[:, None], rtol=1e-5)
        assert np.allclose(d["model_spacing"], sp * np.stack([s, s, np.ones_like(s)], 1), rtol=1e-5)
    with pytest.raises(ValueError, match="scale_range"):
        draw_patch_jobs(pool, 4, torch.Generator().manual_seed(1), **dict(DRAW, scale_range=(1.4, 0.7)))
    with pytest.raises(ValueError, match="fg_prob"):
        draw_patch_jobs(pool, 4, torch.Generator().manual_seed(1), **dict(DRAW, fg_prob=1.5))


def test_foreground_share_is_binomial():
    from dinox.patches import draw_patch_jobs
    pool, _, _ = _pool()
    n, p = 4000, 0.33
    d = draw_patch_jobs(pool, n, torch.Generator().manual_seed(11), **dict(DRAW, fg_prob=p))
    share = float((d["fg_class"] >= 0).mean())
    assert abs(share - p) <= 4 * math.sqrt(p * (1 - p) / n), share
    # a sample whose only class is background still yields jobs, foreground-centred ones on class 0
    assert (d["sample"] == 3).sum() > 500 and set(d["fg_class"][d["sample"] == 3].tolist()) == {-1, 0}


# ------------------------------------------------------------------------------------------ the command line
def _script():
    if "finetune_segmentation" in sys.modules:
        return sys.modules["finetune_segmentation"]
    spec = importlib.util.spec_from_file_location("finetune_segmentation", os.path.join(ROOT, "dino-x_amd", "scripts", "finetune_segmentation.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


BASE = ["--backbone", "/nonexistent/backbone", "--synthetic", "24", "--output", "/nonexistent/out"]


def test_parser_keeps_its_actions_and_patch_flags_parse_through_parse_cli():
    fs = _script()
    assert len(fs.build_parser()._actions) == 31
    with pytest.raises(SystemExit):
        fs.build_parser().parse_args(BASE + ["--patch-train"])
    a = fs.parse_cli(BASE)
    assert (a.patch_train, a.patch_size, a.patch_fg_prob, a.patch_rotate_deg, a.patch_scale, a.patches_per_epoch, a.patch_pool_gib, a.patch_val) == \
        (False, None, 0.33, 15.0, [0.7, 1.4], None, 16.0, "center")
    a = fs.parse_cli(BASE + ["--patch-train", "--patch-size", "96", "--patch-fg-prob", "0.5", "--patch-rotate-deg", "30", "--patch-scale", "0.5", "2",
                             "--patches-per-epoch", "100", "--patch-pool-gib", "2", "--patch-val", "tiled", "--boundary-weight", "0.1"])
    assert (a.patch_train, a.patch_size, a.patch_fg_prob, a.patch_rotate_deg, a.patch_scale, a.patches_per_epoch, a.patch_pool_gib, a.patch_val) == \
        (True, 96, 0.5, 30.0, [0.5, 2.0], 100, 2.0, "tiled") and a.boundary_weight == 0.1 and a.synthetic == 24
    with pytest.raises(SystemExit):
        fs.parse_cli(BASE + ["--patch-val", "sliding"])
    cfg = fs.SegConfig(backbone="b", task="segmentation", num_classes=3, rank=0, alpha=1.0, lr=1e-3, epochs=1, batch_size=2, input_format="float01",
                       scale_aware=False)
    assert (cfg.patch_train, cfg.patch_size, cfg.patch_scale, cfg.patches_per_epoch, cfg.patch_val) == (False, 0, None, 0, "center")


@pytest.mark.parametrize("flags,message", [
    (["--patch-train", "--patch-scale", "1.4", "0.7"], "--patch-scale 1.4 0.7: finite, 0 < LO <= HI"),
    (["--patch-train", "--patch-scale", "0", "1"], "--patch-scale 0.0 1.0: finite, 0 < LO <= HI"),
    (["--patch-train", "--patch-scale", "0.5", "nan"], "--patch-scale 0.5 nan: finite, 0 < LO <= HI"),
    (["--patch-train", "--patch-fg-prob", "1.2"], "--patch-fg-prob 1.2: a probability in [0, 1]"),
    (["--patch-train", "--patch-rotate-deg", "-3"], "--patch-rotate-deg -3.0: degrees in [0, 180]"),
    (["--patch-train", "--patch-size", "0"], "--patch-size 0: the patch side must be >= 1"),
    (["--patch-train", "--patches-per-epoch", "1"], "--patches-per-epoch 1 does not fill one batch of"),
    (["--patch-train", "--patch-pool-gib", "0"], "--patch-pool-gib 0.0: must be > 0"),
    (["--patch-val", "tiled"], "--patch-val tiled belongs to --patch-train")])
def test_bad_patch_settings_are_refused_before_the_backbone_is_looked_for(flags, message, capsys):
    fs = _script()
    args = fs.parse_cli(BASE + flags)                       # the flags parse; run() refuses the values, with its own message
    with pytest.raises(SystemExit):
        fs.run(args)
    assert message in capsys.readouterr().err               # (a missing backbone would raise something else, later)
