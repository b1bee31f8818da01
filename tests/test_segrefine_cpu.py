"""CPU checks of the edge-aware refinement: tests/_segrefine_oracle.py against a float64 framework statement (F.interpolate, F.pad and
shifted slices), the noisy-disc case the feature was motivated by, T = 0 against the calibration oracle, the decided-pixel share of the
GPU cases, the argument refusals of the two C entries and of ops.seg_refine (host checks, nothing is launched), RefineConfig with
load_segmenter, and the new flags of the two scripts."""
import ctypes
import importlib.util
import json
import os
import sys

import numpy as np
import pytest
import torch

import _segcalib_oracle as CO
import _segrefine_oracle as RO
from conftest import ROOT

# the GPU cases (tests/test_segrefine_gpu.py builds its list from these)
GEOS = ((1, 4), (2, 3), (3, 16), (5, 1), (2, 32), (14, 16))
BS = (1, 3)
CS = (2, 5, 33, 64)
TS = (0, 1, 2, 5)
RDS = ((1, 1), (2, 2), (3, 1), (3, 8))
LAMS = (0.0, 0.8, 1.0)
WS = (0.0, 4.0, 20.0)
SS = (1.0, 0.37, 2.5)
SIGMA_XY = (3.0, 1.5, 6.0)
SIGMA_I = (0.5, 0.25, 2.0)


def case_params(i: int) -> dict:
    """The parameters of case i: every list cycles at its own period (4, 4, 3, 3, 3 with shifts), so a few cases meet every value and
    many pairs."""
    r, d = RDS[(i + i // 4) % 4]
    return dict(T=TS[i % 4], r=r, d=d, lam=LAMS[i % 3], w=WS[(i // 3 + i) % 3], s=SS[(i // 2) % 3], sigma_xy=SIGMA_XY[(i // 4) % 3],
                sigma_i=SIGMA_I[(i // 5) % 3])


def refused(p: dict, S: int) -> bool:
    """Windows the entry points refuse at image side S: r d reaches across it, or 2 d > S leaves the middle pixels no neighbour."""
    return p["r"] * p["d"] >= S or 2 * p["d"] > S


def make_guide(rng, B, S):
    return rng.standard_normal((B, S, S)).astype(np.float32)


def normal_case(g, u, B, C, i):
    """Logits (standard normal x 3) and guide (standard normal) of the "normal" regime of case i."""
    rng = np.random.default_rng([41, g, u, B, C, i])
    z = (rng.standard_normal((B, g * g, C)) * 3).astype(np.float32)
    return z, make_guide(rng, B, g * u)


# ------------------------------------------------------------------------------------------ the oracle against the framework
def framework(z, guide, g, u, *, s, T, r, d, sigma_xy, sigma_i, lam, w):
    import torch.nn.functional as F
    s, lam, w = (float(np.float32(v)) for v in (s, lam, w))
    B, C, S, H = z.shape[0], z.shape[2], g * u, r * d
    l = F.interpolate(torch.from_numpy(z).double().reshape(B, g, g, C).permute(0, 3, 1, 2), scale_factor=u, mode="bilinear", align_corners=False)
    U = s * l                                             # [B, C, S, S]
    Q = U.softmax(1)
    I = torch.from_numpy(guide).double()[:, None]
    V = U
    pad = (H, H, H, H)
    for _ in range(T):
        Qp, Ip, ones = F.pad(Q, pad), F.pad(I, pad), F.pad(torch.ones_like(I), pad)
        num, den = torch.zeros_like(Q), torch.zeros_like(I)
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                if dy == 0 and dx == 0:
                    continue
                sl = (slice(None), slice(None), slice(H + dy * d, H + dy * d + S), slice(H + dx * d, H + dx * d + S))
                gj = float(np.exp(-(dy * dy + dx * dx) * d * d / (2.0 * sigma_xy ** 2)))
                a = (1.0 - lam) + lam * torch.exp(-(I - Ip[sl]) ** 2 / (2.0 * sigma_i ** 2))
                num = num + gj * a * ones[sl] * Qp[sl]
                den = den + gj * ones[sl]
        V = U + w * (num / den)
        Q = V.softmax(1)
    return V.permute(0, 2, 3, 1).numpy(), Q.permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize("g,u,C", [(2, 3, 2), (3, 4, 5), (5, 1, 7), (2, 32, 3)])
def test_oracle_against_the_framework(g, u, C):
    for i, B in ((1, 2), (7, 1), (10, 1)):
        p = case_params(i)
        if refused(p, g * u):
            p.update(r=1, d=1)
        p["T"] = max(p["T"], 1)
        z, guide = normal_case(g, u, B, C, i)
        o = RO.refine(z, guide, g, u, **p)
        V, Q = framework(z, guide, g, u, **p)
        assert np.abs(o["V"] - V).max() <= 1e-12 and np.abs(o["Q"] - Q).max() <= 1e-12, (p, np.abs(o["V"] - V).max())
        assert np.array_equal(o["pred"], V.argmax(-1)) and np.abs(o["conf"] - Q.max(-1)).max() <= 1e-12
        assert (o["e_V"] > 0).all() and (o["e_V"] < 1e-3).all() and (o["e_conf"] < 1e-3).all()      # bounds, not blank cheques


def test_the_disc_case_improves():
    z, guide, truth, u = RO.disc_case()
    kw = dict(r=2, d=2, sigma_xy=3.0, sigma_i=0.25, lam=0.8, w=4.0)
    d0, d1, d3, d6 = (RO.dice(RO.refine(z, guide, 8, u, T=T, **kw)["pred"][0], truth) for T in (0, 1, 3, 6))
    msg = f"Dice of the disc: unrefined {d0:.4f}, T = 1 {d1:.4f}, T = 3 {d3:.4f}, T = 6 {d6:.4f}"
    print(msg)
    assert d3 > d0 and d1 > d0, msg
    assert d6 >= d3 - 0.005, msg                           # it stays there


def test_zero_iterations_is_the_calibration_oracle():
    for (g, u), C, s in zip(GEOS[:5], (2, 5, 33, 64, 3), (1.0, 0.37, 2.5, 1.0, 0.37)):
        z, guide = normal_case(g, u, 2, C, 0)
        o = RO.refine(z, guide, g, u, s=s, T=0, r=1, d=1)
        cal = CO.Calib(z, None, g, u)
        c = cal.at(s)
        assert np.array_equal(o["pred"], cal.pred) and np.abs(o["conf"] - c["conf"]).max() <= 1e-15
        assert (o["decided"] <= cal.decided).all()          # twice the bound here, once there


LOGITS = ("normal", "pm80", "dominant")


def logit_regime(i: int) -> str:
    return LOGITS[(i // 4) % 3]


def gpu_cases(g, u, B, C):
    """The case indices (g, u, B, C) runs on the GPU: all 12 at the small geometries (four per logit regime, T cycling inside each).  At
    (14, 16) one per (B, C), chosen so that the float64 oracle stays at seconds and every register width meets the iteration kernel at
    S = 224: C = 2 runs T = 5, C = 5 T = 2, C = 64 T = 1 and C = 33 T = 0.  B = 1 takes cases 0-3 ("normal"), B = 3 cases 4-7 ("pm80")."""
    if g == 14:
        return [(3, 2, 0, 1)[CS.index(C)] + 4 * BS.index(B)]
    return list(range(12))


@pytest.mark.parametrize("g,u", GEOS)
def test_undecided_share_of_the_gpu_cases(g, u):
    """At most 1 % of the pixels of the "normal" regime of the GPU cases, pooled per geometry, have a final top-two gap under twice the
    bound."""
    und = tot = 0
    for B in BS:
        for C in CS:
            for i in gpu_cases(g, u, B, C):
                p = case_params(i)
                if logit_regime(i) != "normal" or refused(p, g * u):
                    continue
                z, guide = normal_case(g, u, B, C, i)
                o = RO.refine(z, guide, g, u, **p)
                und += int((~o["decided"]).sum())
                tot += o["decided"].size
    share = und / max(tot, 1)
    print(f"(g, u) = ({g}, {u}): {und} of {tot} pixels undecided ({share:.4%})")
    assert tot > 0 and share <= 0.01


# ------------------------------------------------------------------------------------------ the C entries refuse on the host
def test_argument_refusal_without_a_gpu():
    from dinox import _lib
    lib, f = _lib.lib, ctypes.c_float
    z, I, y, pred, conf, counts, ws = (ctypes.c_void_p(0x1000 * (i + 1)) for i in range(7))   # never dereferenced: refused before any launch
    tab = np.ones(49, dtype=np.float32)
    good = dict(B=2, g=3, u=4, C=5, T=5, r=2, d=2, inv=2.0, lam=0.8, w=4.0, s=1.0)

    def call(z=z, I=I, y=y, pred=pred, counts=counts, ws=ws, gtab=tab, **kw):
        a = dict(good, **kw)
        return lib.dinox_seg_refine(z, I, y, pred, conf, counts, ws, a["B"], a["g"], a["u"], a["C"], a["T"], a["r"], a["d"],
                                    None if gtab is None else gtab.ctypes.data, f(a["inv"]), f(a["lam"]), f(a["w"]), f(a["s"]), None)

    assert lib.dinox_seg_refine_ws_bytes(2, 3, 4, 5) == 2 * 2 * 5 * 12 * 12 * 4
    # 2 d > S with r d < S: the pixels with S - d <= x, y < d would have an empty neighbourhood and a normaliser of 0
    for kw in (dict(g=1, u=4, r=1, d=3), dict(g=2, u=3, r=1, d=4), dict(g=5, u=1, r=1, d=3), dict(g=3, u=4, r=1, d=8), dict(g=3, u=4, r=1, d=7)):
        assert call(**kw) == -1 and "no neighbour" in _lib.last_error(), (kw, _lib.last_error())
    for kw, word in ((dict(r=3, d=4), "r d"), (dict(r=3, d=8), "r d"), (dict(g=1, u=2, r=1, d=2), "r d"), (dict(T=33), "T=33"), (dict(T=-1), "T=-1"),
                     (dict(r=0), "r=0"), (dict(r=4), "r=4"), (dict(d=0), "d=0"), (dict(d=9), "d=9"), (dict(s=float("nan")), "inv_temperature"),
                     (dict(s=0.0), "inv_temperature"), (dict(s=float("inf")), "inv_temperature"), (dict(w=float("nan")), "w="),
                     (dict(w=-1.0), "w="), (dict(w=float("inf")), "w="), (dict(lam=float("nan")), "lambda"), (dict(lam=1.5), "lambda"),
                     (dict(lam=-0.1), "lambda"), (dict(inv=float("nan")), "sigma_I"), (dict(inv=-1.0), "sigma_I"), (dict(inv=float("inf")), "sigma_I")):
        assert call(**kw) == -1 and word in _lib.last_error(), (kw, _lib.last_error())
    assert call(I=None) == -1 and "null" in _lib.last_error()
    assert call(z=None) == -1 and call(pred=None) == -1 and call(gtab=None) == -1
    assert call(ws=None) == -1 and "ws" in _lib.last_error()
    assert call(y=None) == -1 and "both or neither" in _lib.last_error()
    assert call(counts=None) == -1 and "both or neither" in _lib.last_error()
    for bad in (np.nan, -1.0, np.inf):
        t = tab.copy()
        t[3] = bad
        assert call(gtab=t) == -1 and "gtab[3]" in _lib.last_error()
    t = tab.copy()
    t[2 * 2 * 3 + 1] = 0.0                                  # the neighbour at (0, +1) of r = 2
    assert call(gtab=t) == -1 and "gtab[13]" in _lib.last_error()
    for kw, word in ((dict(C=1), "C=1"), (dict(u=33), "u=33"), (dict(B=0), "B=0"), (dict(g=0), "g=0")):
        assert call(**kw) != 0 and word in _lib.last_error()
        a = dict(good, **kw)
        assert lib.dinox_seg_refine_ws_bytes(a["B"], a["g"], a["u"], a["C"]) == 0
    assert call(C=65) == -2 and lib.dinox_seg_refine_ws_bytes(2, 3, 4, 65) == 0
    assert lib.dinox_seg_refine_ws_bytes(1 << 20, 4096, 32, 2) == 0 and call(B=1 << 20, g=64, u=32) == -1      # beyond the tile and plane limits
    assert lib.dinox_version() == 3


def test_ops_refuses_before_the_device():
    from dinox import ops
    z, guide = torch.zeros((1, 4, 3)), torch.zeros((1, 8, 8))
    for kw, word in ((dict(iters=33), "iters"), (dict(iters=-1), "iters"), (dict(iters=2.0), "iters"), (dict(radius=0), "radius"), (dict(radius=4), "radius"),
                     (dict(dilation=0), "dilation"), (dict(dilation=9), "dilation"), (dict(radius=3, dilation=3), "no neighbour"), (dict(radius=1, dilation=5), "no neighbour"),
                     (dict(sigma_xy=0.0), "sigma_xy"), (dict(sigma_xy=float("nan")), "sigma_xy"), (dict(sigma_xy=0.01), "every spatial weight"),
                     (dict(sigma_i=0.0), "sigma_i"), (dict(sigma_i=float("inf")), "sigma_i"), (dict(sigma_i=1e-30), "sigma_i"),
                     (dict(mix=1.1), "mix"), (dict(mix=float("nan")), "mix"), (dict(weight=-1.0), "weight"), (dict(weight=float("nan")), "weight"),
                     (dict(inv_temperature=0.0), "inv_temperature"), (dict(inv_temperature=1e-60), "inv_temperature")):
        with pytest.raises(ValueError, match=word):
            ops.seg_refine(z, guide, 4, **kw)
    with pytest.raises(ValueError, match="guide must be fp32"):
        ops.seg_refine(z, torch.zeros((1, 8, 9)), 4)
    with pytest.raises(ValueError, match="guide must be fp32"):
        ops.seg_refine(z, guide.double(), 4)
    with pytest.raises(ValueError, match="do not have side"):
        ops.seg_refine(z, guide, 4, torch.zeros((1, 4, 4), dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        ops.seg_refine(z, guide, 4)                         # the arguments are fine: only the device is missing
    t = ops.seg_refine_table(1, 2, 3.0)
    assert t.dtype == np.float32 and t.shape == (9,) and t[4] == 1.0 and t[5] == np.float32(np.exp(-4 / 18)) and t[0] == np.float32(np.exp(-8 / 18))


# ------------------------------------------------------------------------------------------ RefineConfig, load_segmenter, the scripts
def test_refine_config_round_trip():
    from dinox.segment import RefineConfig
    d = RefineConfig()
    assert d.to_dict() == dict(iters=5, radius=2, dilation=2, sigma_xy=3.0, sigma_i=0.5, mix=0.8, weight=4.0)
    c = RefineConfig(iters=3, radius=1, dilation=4, sigma_xy=2.0, sigma_i=0.1, mix=1.0, weight=0.0)
    assert RefineConfig.from_dict(c.to_dict()) == c and RefineConfig.from_dict(json.loads(json.dumps(c.to_dict()))) == c
    assert RefineConfig.from_dict({"iters": 2}) == RefineConfig(iters=2)
    with pytest.raises(ValueError, match="unknown"):
        RefineConfig.from_dict({"iterations": 2})
    for kw in (dict(iters=33), dict(radius=0), dict(dilation=9), dict(sigma_xy=0.0), dict(sigma_i=float("nan")), dict(mix=2.0), dict(weight=-1.0),
               dict(iters=True), dict(radius=1.5)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            RefineConfig(**kw)


def test_load_segmenter_reads_refine(tmp_path, monkeypatch):
    import zoo.arch as arch
    import zoo.hub
    from dinox import segment as SG
    from test_segloss_gpu import TINY
    monkeypatch.setattr(zoo.hub, "load_model", lambda path, device="cpu": arch.PatchViT(**TINY))
    head = SG.SegHead(TINY["dim"], 3)
    torch.save(head.state_dict(), tmp_path / SG.HEAD_FILE)
    cfg = {"task": "segmentation", "rank": 0, "num_classes": 3}
    (tmp_path / SG.CONFIG_FILE).write_text(json.dumps(cfg))
    m = SG.load_segmenter("unused", tmp_path, "cpu")
    assert m.refine is None and m.temperature == 1.0
    want = SG.RefineConfig(iters=2, sigma_i=0.25)
    (tmp_path / SG.CONFIG_FILE).write_text(json.dumps(dict(cfg, refine=want.to_dict(), temperature=1.5)))
    m = SG.load_segmenter("unused", tmp_path, "cpu")
    assert m.refine == want and m.temperature == 1.5
    (tmp_path / SG.CONFIG_FILE).write_text(json.dumps(dict(cfg, refine={"radius": 7})))
    with pytest.raises(ValueError, match="radius"):
        SG.load_segmenter("unused", tmp_path, "cpu")


def test_segment_refuses_entropy_with_refine():
    from dinox import segment as SG
    with pytest.raises(ValueError, match="return_entropy"):
        SG.segment(None, np.zeros((8, 8), np.float32), refine=SG.RefineConfig(), return_entropy=True)
    with pytest.raises(ValueError, match="return_entropy"):
        SG.segment_volume(None, np.zeros((2, 8, 8), np.float32), refine=SG.RefineConfig(), return_entropy=True)
    with pytest.raises(ValueError, match="RefineConfig"):
        SG.segment(None, np.zeros((8, 8), np.float32), refine={"iters": 2})


def _script(name):
    if name in sys.modules:
        return sys.modules[name]
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "dino-x_amd", "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


REFINE_FLAGS = ["--refine-iters", "3", "--refine-radius", "1", "--refine-dilation", "4", "--refine-sigma-xy", "2", "--refine-sigma-i", "0.1",
                "--refine-mix", "1", "--refine-weight", "7"]


def test_evaluate_segmentation_flags(capsys):
    from dinox.segment import RefineConfig
    es = _script("evaluate_segmentation")
    ap = es.build_parser()
    base = ["--backbone", "b", "--segmenter", "s", "--synthetic", "8"]
    a = ap.parse_args(base)
    es.check_args(ap, a)
    assert a.refine is False and a.write_refine is False and es.refine_config(a, None) is None
    a = ap.parse_args(base + ["--refine"])
    es.check_args(ap, a)
    assert es.refine_config(a, None) == RefineConfig()
    stored = RefineConfig(iters=9, weight=1.0)
    assert es.refine_config(a, stored) == stored            # the stored parameters are the defaults of the flags
    assert es.refine_config(a, stored.to_dict(), ap) == stored                      # as finetune_config.json holds them
    for bad in ({"radius": 7}, {"iterations": 2}):          # a bad stored object is an argument error, not a traceback
        with pytest.raises(SystemExit) as e:
            es.refine_config(a, bad, ap)
        assert e.value.code == 2 and "--refine: RefineConfig" in capsys.readouterr().err
    with pytest.raises(ValueError, match="radius"):
        es.refine_config(a, {"radius": 7})
    a = ap.parse_args(base + ["--refine", "--write-refine"] + REFINE_FLAGS)
    es.check_args(ap, a)
    assert es.refine_config(a, stored) == RefineConfig(iters=3, radius=1, dilation=4, sigma_xy=2.0, sigma_i=0.1, mix=1.0, weight=7.0)
    for bad, word in ((["--write-refine"], "--write-refine needs --refine"), (["--refine-iters", "3"], "only with --refine"),
                      (["--refine", "--refine-radius", "4"], "radius"), (["--refine", "--refine-mix", "2"], "mix")):
        with pytest.raises(SystemExit) as e:
            es.check_args(ap, ap.parse_args(base + bad))
        assert e.value.code == 2 and word in capsys.readouterr().err


def test_segment_volume_flags(capsys):
    from dinox.segment import RefineConfig
    sv = _script("segment_volume")
    ap = sv.build_parser()
    base = ["--backbone", "b", "--segmenter", "s", "--volume", "v.npy", "--spacing", "1", "1", "1", "--out", "o.npy"]
    a = ap.parse_args(base)
    sv.check_args(ap, a)
    assert a.refine is False
    a = ap.parse_args(base + ["--refine", "--confidence-out", "c.npy"] + REFINE_FLAGS)
    sv.check_args(ap, a)
    assert sv.refine_config(a, None) == RefineConfig(iters=3, radius=1, dilation=4, sigma_xy=2.0, sigma_i=0.1, mix=1.0, weight=7.0)
    for bad, word in ((["--tiled", "--refine"], "--refine: not with --tiled"), (["--refine", "--entropy-out", "e.npy"], "--entropy-out: not with --refine"),
                      (["--refine-weight", "2"], "only with --refine"), (["--refine", "--refine-dilation", "9"], "dilation")):
        with pytest.raises(SystemExit) as e:
            sv.check_args(ap, ap.parse_args(base + bad))
        assert e.value.code == 2 and word in capsys.readouterr().err
