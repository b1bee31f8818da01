"""CPU tests of the sliding-window path: the host logic of dinox/tiled.py and preprocess.volume_tile_jobs, the refusals of
ops.seg_blend_predict (before the library is touched) and of the C entry (before any launch), the oracle's self-tests -- its fp32
emulation of the kernel's arithmetic stays inside the derived bounds on every seeded case of the GPU tests, and every planted defect is
flagged -- and the new flags of scripts/segment_volume.py.

Share of pixels exempted by the margin rule over the 28 seeded cases (cap 1e-3 per case): 0 in 25 cases, 5.1e-4 (three pixels of 5883)
in the largest of the other three (0-64, 1-2, 4-64); the emulation's conf error never passes 4 % of its bound."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

import _segblend_cases as K
import _segblend_oracle as O
from conftest import ROOT


# ------------------------------------------------------------------------------------------ tile_starts / blend_window
@pytest.mark.parametrize("overlap", [0.0, 0.5, 0.75])
@pytest.mark.parametrize("L,t", [(37, 16), (53, 16), (37, 10), (9, 7), (23, 7), (70, 3), (17, 16), (512, 224), (16, 16), (1, 1), (1000, 1)])
def test_tile_starts_cover_the_axis(L, t, overlap):
    from dinox.segment import tile_starts
    s = tile_starts(L, t, overlap)
    step = max(1, int(round(t * (1 - overlap))))
    assert s[0] == 0 and s[-1] == L - t and all(isinstance(v, int) for v in s)
    assert len(s) == (1 if L <= t else -(-(L - t) // step) + 1)
    d = np.diff(s)
    assert (d >= 1).all() and (d <= min(step, t)).all()                             # ascending, no gap: [0, L) is covered
    covered = np.zeros(L, bool)
    for o in s:
        covered[o:o + t] = True
    assert covered.all()
    # evenly spread: no origin is further than half a pixel from i (L - t) / (n - 1)
    if len(s) > 1:
        assert np.abs(np.asarray(s) - np.arange(len(s)) * (L - t) / (len(s) - 1)).max() <= 0.5


def test_tile_starts_edges_and_refusals():
    from dinox.segment import tile_starts
    assert tile_starts(16, 16, 0.5) == [0] and tile_starts(17, 16, 0.5) == [0, 1] and tile_starts(17, 16, 0.0) == [0, 1]
    assert tile_starts(512, 224, 0.5) == [0, 96, 192, 288] and tile_starts(9, 3, 0.0) == [0, 3, 6]
    for bad in ((8, 9, 0.5), (8, 0, 0.5), (8, 4, 1.0), (8, 4, -0.1), (8, 4, float("nan")), (8.5, 4, 0.5), (True, 1, 0.5)):
        with pytest.raises(ValueError, match="tile_starts"):
            tile_starts(*bad)


def test_blend_window():
    from dinox.segment import blend_window
    for t in (1, 2, 3, 7, 16, 224):
        w = blend_window(t, "gaussian")
        assert w.dtype == np.float32 and w.shape == (t,) and np.array_equal(w, w[::-1]) and (w > 0).all() and w.max() <= 1
        d = np.arange(t, dtype=np.float64) - (t - 1) / 2
        assert np.array_equal(w, np.exp(-d * d / (2 * (0.125 * t) ** 2)).astype(np.float32))
        assert np.array_equal(blend_window(t, "constant"), np.ones(t, np.float32))
    assert 5e-8 < float(blend_window(224).min()) ** 2 < 5e-7                        # the smallest weight product: far above underflow
    assert blend_window(7)[3] == 1.0
    with pytest.raises(ValueError, match="zero in fp32"):
        blend_window(64, "gaussian", 0.01)                                          # exp(-1250) = 0
    with pytest.raises(ValueError, match="zero in fp32"):
        blend_window(64, "gaussian", 0.05)                                          # exp(-50) ~ 2e-22 > 0, but its square underflows
    for bad in (dict(kind="hann"), dict(t=0), dict(sigma_scale=0.0), dict(sigma_scale=float("inf"))):
        with pytest.raises(ValueError):
            blend_window(**dict(dict(t=8, kind="gaussian"), **bad))


# ------------------------------------------------------------------------------------------ preprocess.volume_tile_jobs
@pytest.mark.parametrize("context", ["neighbours", "replicate"])
def test_volume_tile_jobs(context):
    from dinox import preprocess as P
    Z, H, W, t = 5, 40, 56, 16
    items = [(0, 0, 0), (0, H - t, W - t), (Z - 1, 0, 8), (Z - 1, H - t, W - t), (2, 3, 5), (2, 3, 5)]      # first / last slice, the corner, a repeat
    jobs = P.volume_tile_jobs(Z, H, W, items, t, context)
    assert P.check_jobs(jobs, Z * H * W, len(items)) == t
    assert (jobs[:, 1] == t).all() and (jobs[:, 2] == t).all() and (jobs[:, 3] == W).all() and (jobs[:, 4] == 1).all()
    # every (image, channel) destination is written exactly once, from the plane its stack shows there, at the tile's origin
    seen = {}
    for off, _, _, _, _, nd, *d in jobs.tolist():
        for dest in d[:nd]:
            assert dest not in seen
            seen[dest] = off
    assert sorted(seen) == list(range(3 * len(items)))
    for k, (z, y0, x0) in enumerate(items):
        for c, plane in enumerate(P.stack_planes(Z, z, context)):
            assert seen[3 * k + c] == plane * H * W + y0 * W + x0
    assert int((jobs[:, 0] + (t - 1) * W + (t - 1)).max()) == Z * H * W - 1          # the corner tile of the last slice ends on the last element
    # one job per distinct plane crop: the repeated item shares its jobs, a clamped stack shows a plane twice
    crops = {(p, y0, x0) for z, y0, x0 in items for p in P.stack_planes(Z, z, context)}
    assert len({int(o) for o in jobs[:, 0]}) == len(crops)
    # the gathered crop is the tile
    vol = np.arange(Z * H * W, dtype=np.int64).reshape(Z, H, W)
    off, th, tw, rs, ps = jobs[-1, :5]
    got = vol.reshape(-1)[off + rs * np.arange(th)[:, None] + ps * np.arange(tw)[None, :]]
    z, rem = divmod(int(off), H * W)
    assert np.array_equal(got, vol[z, rem // W:rem // W + t, rem % W:rem % W + t])


def test_volume_tile_jobs_refusals():
    from dinox import preprocess as P
    for items, t in (([(0, 25, 0)], 16), ([(0, 0, 41)], 16), ([(5, 0, 0)], 16), ([(-1, 0, 0)], 16), ([(0, -1, 0)], 16), ([(0, 0, 0)], 41), ([(0, 0, 0)], 0)):
        with pytest.raises(ValueError):
            P.volume_tile_jobs(5, 40, 56, items, t)
    with pytest.raises(ValueError, match="context"):
        P.volume_tile_jobs(5, 40, 56, [(0, 0, 0)], 16, "mirror")
    jobs = P.volume_tile_jobs(5, 40, 56, [(4, 24, 40)], 16)
    with pytest.raises(ValueError, match="reaches past the source buffer"):
        P.check_jobs(jobs, 5 * 40 * 56 - 1, 1)                                      # a table that reaches past the volume


# ------------------------------------------------------------------------------------------ ops.seg_blend_predict: refusals on the host
def test_ops_refuses_before_the_library(monkeypatch):
    from dinox import ops

    def touched(*a, **k):
        raise AssertionError("the library was called")

    monkeypatch.setattr(ops.lib, "dinox_seg_blend_predict", touched)
    H, W, t, g, C = 20, 24, 8, 2, 3
    ys, xs = [0, 6, 12], [0, 8, 16]
    ok = dict(z=torch.zeros(2, 1, 3, 3, g * g, C), ys=ys, xs=xs, flips=[0], win=np.ones(t, np.float32), H=H, W=W, t=t)
    lab = torch.zeros(2, H, W, dtype=torch.uint8)
    cases = [
        (dict(z=torch.zeros(2, 3, 3, g * g, C)), "tile logits must be"), (dict(z=torch.zeros(2, 1, 3, 3, g * g, C, dtype=torch.int32)), "tile logits must be"),
        (dict(z=np.zeros((2, 1, 3, 3, 4, 3), np.float32)), "tile logits must be"),
        (dict(z=torch.zeros(2, 1, 3, 3, 5, C)), "not a square grid"), (dict(z=torch.zeros(2, 1, 3, 3, 4, 1)), "C must lie"),
        (dict(z=torch.zeros(2, 1, 3, 3, 4, 65)), "C must lie"), (dict(z=torch.zeros(0, 1, 3, 3, 4, 3)), "T = B F ny nx"),
        (dict(z=torch.zeros(2, 5, 3, 3, 4, 3), flips=[0, 1, 2, 3, 0]), "flip variants"), (dict(z=torch.zeros(2, 0, 3, 3, 4, 3), flips=[]), "flip variants"),
        (dict(t=0), "t must be an integer"), (dict(t=8.0), "t must be an integer"), (dict(H=True), "H must be an integer"), (dict(W=(1 << 20) + 1), "W must be"),
        (dict(t=21, win=np.ones(21, np.float32)), "exceeds min"),
        (dict(ys=[0, 6]), "entries"), (dict(xs=[0, 8, 16, 16]), "entries"), (dict(flips=[0, 1]), "entries"),
        (dict(ys=[1, 6, 12]), "ys must start at 0"), (dict(ys=[0, 6, 11]), "ys must start at 0 and end at 20 - 8"), (dict(xs=[0, 8, 15]), "xs must start at 0"),
        (dict(ys=[0, 12, 12]), "strictly ascending"), (dict(ys=[0, 13, 12]), "strictly ascending"), (dict(ys=[0, 3, 12]), "ys leave a gap"),
        (dict(xs=[0, 7, 16]), "xs leave a gap"), (dict(ys=[0.0, 6.0, 12.0]), "ys must be a 1-D"), (dict(xs=[[0, 8, 16]]), "xs must be a 1-D"),
        (dict(ys=[0, 6, 1 << 40]), "outside int32"),
        (dict(flips=[4]), "flip codes"), (dict(flips=[-1]), "flip codes"), (dict(flips=[0.0]), "flips must be a 1-D"),
        (dict(win=np.ones(7, np.float32)), "win must hold"), (dict(win=np.zeros(t, np.float32)), "win must hold"),
        (dict(win=np.full(t, np.nan, np.float32)), "win must hold"), (dict(win=-np.ones(t, np.float32)), "win must hold"), (dict(win=[1] * t), "win must be a 1-D"),
        (dict(labels=lab.float()), "labels must be uint8"), (dict(labels=lab[:, :, :5]), "labels must be uint8"), (dict(labels=lab[:1]), "labels must be uint8"),
    ]
    for kw, msg in cases:
        with pytest.raises(ValueError, match=msg):
            ops.seg_blend_predict(**dict(ok, **kw))
    with pytest.raises(RuntimeError, match="no CPU fallback"):                      # everything is in order: only the device is missing
        ops.seg_blend_predict(**ok)


def test_c_entry_checks_its_arguments_before_any_launch():
    from dinox import _lib
    lib = _lib.lib
    p = 0x1000                                     # never dereferenced: every call below is refused on the host
    ok = dict(z=p, ys=p, xs=p, flips=p, win=p, y=None, pred=p, conf=None, counts=None, B=2, F=1, ny=3, nx=3, g=2, t=8, C=3, H=20, W=24)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.dinox_seg_blend_predict(a["z"], a["ys"], a["xs"], a["flips"], a["win"], a["y"], a["pred"], a["conf"], a["counts"], a["B"], a["F"],
                                           a["ny"], a["nx"], a["g"], a["t"], a["C"], a["H"], a["W"], None)

    for name in ("z", "ys", "xs", "flips", "win", "pred"):
        assert call(**{name: None}) == -1 and "seg_blend_predict: null pointer" in _lib.last_error(), name
    assert call(y=p) == -1 and "both or neither" in _lib.last_error()
    assert call(counts=p) == -1 and "both or neither" in _lib.last_error()
    for kw, msg in ((dict(F=0), "F=0"), (dict(F=5), "F=5"), (dict(B=0), "B=0"), (dict(ny=0), "ny=0"), (dict(nx=0), "nx=0"), (dict(B=(1 << 20) + 1), "B=1048577"),
                    (dict(g=0), "g=0"), (dict(g=4097), "g=4097"), (dict(H=0), "H=0"), (dict(W=(1 << 20) + 1), "W=1048577"), (dict(t=0), "t=0"),
                    (dict(t=21), "t=21"), (dict(t=25, H=30), "t=25"), (dict(C=1), "C=1"), (dict(t=1 << 17, g=4096, H=1 << 17, W=1 << 17), "t g"),
                    (dict(B=1 << 20, H=1 << 20, W=64), "runs")):
        assert call(**kw) == -1 and msg in _lib.last_error() and "seg_blend_predict" in _lib.last_error(), (kw, _lib.last_error())
    assert call(C=65) == _lib.EUNSUPPORTED and "at most 64" in _lib.last_error()


# ------------------------------------------------------------------------------------------ the oracle's self-tests
@pytest.mark.parametrize("cid", K.case_ids())
def test_emulation_stays_inside_the_bounds_on_every_gpu_case(cid):
    """The fp32 emulation of the kernel's arithmetic over the exact seeded inputs of the GPU tests: arg-max, conf bound, and the share of
    pixels the margin rule exempts under its cap -- established here, without a GPU, before the GPU tests rely on it."""
    s, ys, xs, win, z, want = K.case(cid)
    pred, conf = O.emulate(z, ys, xs, s["flips"], win, s["H"], s["W"], s["t"])
    share, worst = want.check(pred, conf)
    assert share <= 1e-3 and worst <= 1.0
    print(f"{cid}: {s}: exempt share {share:.2e}, conf error / bound {worst:.3f}")


SELF = dict(H=21, W=27, t=10, g=4, C=3, B=2)


def _self_case(flips, window="gaussian", seed=5):
    from dinox.tiled import blend_window, tile_starts
    ys, xs = tile_starts(SELF["H"], SELF["t"], 0.5), tile_starts(SELF["W"], SELF["t"], 0.5)
    win = blend_window(SELF["t"], window)
    z = O.make_logits("randn", (SELF["B"], len(flips), len(ys), len(xs), SELF["g"] ** 2, SELF["C"]), seed)
    return ys, xs, win, z, O.Blend(z, ys, xs, flips, win, SELF["H"], SELF["W"], SELF["t"])


@pytest.mark.parametrize("defect", O.DEFECTS)
def test_oracle_flags_every_planted_defect(defect):
    flips = [0, 3, 1, 2]
    ys, xs, win, z, want = _self_case(flips)
    want.check(*O.emulate(z, ys, xs, flips, win, SELF["H"], SELF["W"], SELF["t"]))  # the faithful emulation passes ...
    with pytest.raises(AssertionError):                                             # ... and the defective one does not
        want.check(*O.emulate(z, ys, xs, flips, win, SELF["H"], SELF["W"], SELF["t"], defect=defect))


def test_oracle_statement_against_a_pixel_loop():
    """The vectorised float64 statement against the definition read pixel by pixel (a loop over pixels, variants and tiles)."""
    flips = [2, 1]
    ys, xs, win, z, want = _self_case(flips, seed=6)
    t, g, H, W = SELF["t"], SELF["g"], SELF["H"], SELF["W"]
    w64 = win.astype(np.float64)
    rng = np.random.default_rng(0)
    for y, x in [(0, 0), (H - 1, W - 1), (0, W - 1), (H - 1, 0)] + [(int(rng.integers(H)), int(rng.integers(W))) for _ in range(40)]:
        num, den = np.zeros(SELF["C"]), 0.0
        for f, code in enumerate(flips):
            for iy, y0 in enumerate(ys):
                for ix, x0 in enumerate(xs):
                    ly, lx = y - y0, x - x0
                    if not (0 <= ly < t and 0 <= lx < t):
                        continue
                    ly = t - 1 - ly if code & 2 else ly
                    lx = t - 1 - lx if code & 1 else lx
                    sy, sx = max((ly + 0.5) * g / t - 0.5, 0.0), max((lx + 0.5) * g / t - 0.5, 0.0)
                    ky, kx = int(np.floor(sy)), int(np.floor(sx))
                    ky1, kx1 = min(ky + 1, g - 1), min(kx + 1, g - 1)
                    zt = z[1, f, iy, ix].astype(np.float64).reshape(g, g, -1)
                    fy, fx = sy - ky, sx - kx
                    l = (1 - fy) * ((1 - fx) * zt[ky, kx] + fx * zt[ky, kx1]) + fy * ((1 - fx) * zt[ky1, kx] + fx * zt[ky1, kx1])
                    w = w64[ly] * w64[lx]
                    num, den = num + w * l, den + w
        assert np.allclose(want.L[1, y, x], num / den, rtol=1e-12, atol=1e-12)
    # the integer form of the fraction the kernel uses is the same number
    for mirror in (False, True):
        lm, k0, k1, w1 = O.axis_taps(t, g, mirror)
        n = (2 * lm + 1) * g - t
        assert np.array_equal(k0, np.where(n > 0, n // (2 * t), 0))
        assert np.allclose(np.where((k0 + 1 < g) & (n > 0), (n - 2 * t * k0) / (2 * t), 0.0), np.where(k1 > k0, w1, 0.0), atol=1e-15)


def test_oracle_mirrored_variants_blend_to_the_first():
    """Mirror identity of the statement itself: variants that hold the mirrored logits of variant 0 leave every blended logit where F = 1
    puts it (the window is symmetric)."""
    from dinox.tiled import blend_window, tile_starts
    ys, xs, win = tile_starts(21, 10, 0.5), tile_starts(27, 10, 0.5), blend_window(10, "gaussian")
    z0 = O.make_logits("randn", (2, len(ys), len(xs), 16, 3), 9)
    flips = [0, 2, 3, 1]
    one = O.Blend(z0[:, None], ys, xs, [0], win, 21, 27, 10)
    four = O.Blend(O.mirrored_variants(z0, flips), ys, xs, flips, win, 21, 27, 10)
    assert np.allclose(one.L, four.L, rtol=0, atol=1e-12)


def test_confusion_counts():
    pred = np.array([[0, 1, 2, 1]], np.uint8)
    lab = np.array([[0, 2, 2, 255]], np.uint8)
    assert O.confusion_counts(pred, lab, 3).tolist() == [[1, 0, 1], [1, 1, 1], [1, 0, 2]]


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


def test_script_tiled_flags(capsys):
    sv = _script()
    ap = sv.build_parser()
    a = ap.parse_args(BASE)
    sv.check_args(ap, a)
    assert (a.tiled, a.tta_flips, a.tile, a.overlap, a.blend_window) == (False, False, None, 0.5, "gaussian")
    assert (a.context, a.batch_size, a.keep_largest, a.min_component_mm3, a.connectivity, a.labels, a.report) == \
        ("neighbours", 64, False, 0.0, 26, None, None)                              # the old defaults
    a = ap.parse_args(BASE + ["--tiled"])
    sv.check_args(ap, a)
    assert (a.tiled, a.tta_flips, a.tile, a.overlap, a.blend_window) == (True, False, None, 0.5, "gaussian")
    a = ap.parse_args(BASE + ["--tiled", "--tile", "96", "--overlap", "0.75", "--blend-window", "constant", "--tta-flips"])
    sv.check_args(ap, a)
    assert (a.tiled, a.tta_flips, a.tile, a.overlap, a.blend_window) == (True, True, 96, 0.75, "constant")
    for extra, flag in ((["--tile", "96"], "--tile"), (["--overlap", "0.5"], "--overlap"), (["--blend-window", "gaussian"], "--blend-window"),
                        (["--tta-flips"], "--tta-flips")):
        with pytest.raises(SystemExit):
            sv.check_args(ap, ap.parse_args(BASE + extra))
        err = capsys.readouterr().err
        assert flag in err and "only with --tiled" in err
    for extra, msg in ((["--overlap", "1.0"], "--overlap"), (["--overlap", "-0.1"], "--overlap"), (["--tile", "0"], "--tile")):
        with pytest.raises(SystemExit):
            sv.check_args(ap, ap.parse_args(BASE + ["--tiled"] + extra))
        assert msg in capsys.readouterr().err
    with pytest.raises(SystemExit):
        ap.parse_args(BASE + ["--tiled", "--blend-window", "hann"])
    capsys.readouterr()


def test_script_native_labels(tmp_path, capsys):
    sv = _script()
    ap = sv.build_parser()
    gt = np.random.default_rng(0).integers(0, 3, size=(2, 12, 10)).astype(np.uint8)
    np.save(tmp_path / "gt.npy", gt)
    np.save(tmp_path / "grid.npy", gt[:, :8, :8].copy())
    assert np.array_equal(sv.native_labels(ap, tmp_path / "gt.npy", (2, 12, 10)), gt)
    with pytest.raises(SystemExit):
        sv.native_labels(ap, tmp_path / "grid.npy", (2, 12, 10))                    # the model's grid is not the series': nothing is resampled
    assert "with --tiled" in capsys.readouterr().err
