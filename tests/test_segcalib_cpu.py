"""CPU checks of the segmentation calibration path: tests/_segcalib_oracle.py against the float64 framework statement (F.interpolate,
log_softmax, autograd in s, ECE by torch.bucketize), dinox.segment.calibration_report on hand-built integer tables, the Newton /
bisection logic of dinox.segment.fit_temperature with the oracle standing in for the kernel, the argument refusals of the two C entries
(host checks, nothing is launched) and the new flags of the three scripts."""
import ctypes
import importlib.util
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _segcalib_oracle as CO
from conftest import ROOT


def _case(seed, B, g, u, C, scale=3.0, ignore=0.25):
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal((B, g * g, C)) * scale).astype(np.float32)
    y = rng.integers(0, C, (B, g * u, g * u)).astype(np.uint8)
    y[rng.random(y.shape) < ignore] = 255
    return z, y


# ------------------------------------------------------------------------------------------ the oracle against the framework
@pytest.mark.parametrize("g,u,B,C,s", [(2, 3, 2, 5, 1.0), (3, 4, 1, 2, 0.37), (5, 1, 2, 7, 2.5), (2, 32, 1, 3, 2.5)])
def test_oracle_against_the_framework(g, u, B, C, s):
    import torch.nn.functional as F
    z, y = _case([1, g, u, C], B, g, u, C)
    o = CO.Calib(z, y, g, u).at(s)
    s = o["s"]
    l = F.interpolate(torch.from_numpy(z).double().reshape(B, g, g, C).permute(0, 3, 1, 2), scale_factor=u, mode="bilinear", align_corners=False)
    sv = torch.tensor(s, dtype=torch.float64, requires_grad=True)
    logp = (sv * l).log_softmax(1)
    p = logp.exp()
    yl = torch.from_numpy(y).long()
    valid = yl != 255
    pred = l.argmax(1)
    conf = p.gather(1, pred[:, None])[:, 0]
    ent = -(p * logp).sum(1) / math.log(C)
    nll = F.nll_loss(logp, yl, ignore_index=255, reduction="sum")
    (G,) = torch.autograd.grad(nll, sv, create_graph=True)
    (H,) = torch.autograd.grad(G, sv)
    oh = F.one_hot(torch.where(valid, yl, 0), C).permute(0, 3, 1, 2).double()
    brier = (((p - oh) ** 2).sum(1) * valid).sum()
    assert np.array_equal(pred.numpy(), CO.Calib(z, y, g, u).pred)
    assert np.allclose(conf.detach().numpy(), o["conf"], rtol=0, atol=1e-12)
    assert np.allclose(ent.detach().numpy(), o["entropy"], rtol=0, atol=1e-12)
    want = [float(v.detach()) for v in (nll, brier, G, H, (ent * valid).sum())]
    assert np.allclose(o["sums"], want, rtol=1e-11, atol=1e-9), (o["sums"], want)
    n3 = CO.Calib(z, y, g, u).newton(s)
    assert np.allclose(n3, [want[0], want[2], want[3]], rtol=1e-11, atol=1e-9)
    assert (o["e_sums"] > 0).all() and (o["e_sums"] < 1e-2 * (np.abs(o["sums"]) + valid.sum().item())).all()      # bounds, not blank cheques

    # ECE by hand with torch.bucketize against histogram() + calibration_report()
    from dinox.segment import calibration_report
    NB = 10
    c32 = conf.detach().float()
    hist, tail = CO.histogram(pred.numpy(), c32.numpy(), y, C, NB)
    rep = calibration_report(hist, tail, o["sums"])
    edges = torch.linspace(0, 1, NB + 1, dtype=torch.float64)
    k = torch.bucketize(c32.double(), edges[1:-1], right=True)
    hit = (pred == yl).double()
    ece, N = 0.0, int(valid.sum())
    for b in range(NB):
        sel = valid & (k == b)
        if sel.any():
            ece += abs(float(hit[sel].sum()) - float(c32.double()[sel].sum())) / N
    assert rep["pixels"] == N == sum(b["count"] for b in rep["bins"] if b)
    assert abs(rep["ece"] - ece) <= 2.0 ** -24                 # the fixed point rounds each confidence by at most 2^-25
    assert abs(rep["nll"] - want[0] / N) <= 1e-12 and abs(rep["accuracy"] - float(hit[valid].mean())) <= 1e-12


def test_undecided_share_of_the_new_gpu_shapes():
    """The GPU test holds conf / entropy to the oracle where the float64 arg-max is decided (margin > e_l) and asserts that at most 1 % of
    the pixels of the "normal" logits are not; tests/test_segloss_gpu.py holds its generators to that at its own shapes, this is the same
    for the two geometries the calibration tests add."""
    for g, u in ((5, 1), (2, 32)):
        for B in (1, 3):
            for C in (2, 5, 33, 64):
                rng = np.random.default_rng([11, g, u, B, C])
                z = (rng.standard_normal((B, g * g, C)) * 3).astype(np.float32)
                cal = CO.Calib(z, None, g, u)
                assert 1.0 - cal.decided.mean() <= 0.01, (g, u, B, C)


# ------------------------------------------------------------------------------------------ calibration_report
def test_report_on_hand_built_tables():
    from dinox.segment import Q_ONE, CalibrationAccumulator, calibration_report
    assert Q_ONE == 1 << 24
    # perfectly calibrated: correct / count == Q / (2^24 count) in every bin
    hist = [[8, 1, Q_ONE], [0, 0, 0], [4, 2, 2 * Q_ONE], [3, 3, 3 * Q_ONE]]
    rep = calibration_report(torch.tensor(hist), torch.tensor([15, 0, 0]), torch.tensor([30.0, 7.5, 0.0, 1.0, 3.0], dtype=torch.float64))
    assert rep["ece"] == 0.0 and rep["mce"] == 0.0 and rep["bins"][1] is None
    assert rep["bins"][0] == {"count": 8, "accuracy": 0.125, "mean_confidence": 0.125}
    assert (rep["pixels"], rep["nll"], rep["brier"], rep["mean_entropy"], rep["accuracy"], rep["mean_confidence"]) == (15, 2.0, 0.5, 0.2, 0.4, 0.4)
    # one bin, 7 of 10 right at confidence 0.9
    rep = calibration_report(np.array([[10, 7, 9 * Q_ONE]]), np.array([10, 0, 0]), np.zeros(5))
    assert rep["ece"] == 0.2 and rep["mce"] == 0.2 and rep["accuracy"] == 0.7 and rep["mean_confidence"] == 0.9
    # non-finite pixels are outside N
    rep = calibration_report([[2, 2, Q_ONE]], [5, 0, 3], [1.0, 1.0, 0.0, 0.0, 1.0])
    assert rep["pixels"] == 2 and rep["nonfinite"] == 3 and rep["nll"] == 0.5 and rep["ece"] == 0.5
    # nothing valid
    rep = calibration_report(torch.zeros((15, 3), dtype=torch.int64), torch.zeros(3, dtype=torch.int64), torch.zeros(5))
    assert rep["pixels"] == 0 and all(b is None for b in rep["bins"])
    assert all(rep[k] is None for k in ("ece", "mce", "nll", "brier", "mean_entropy", "accuracy", "mean_confidence"))
    with pytest.raises(ValueError, match="bins hold"):
        calibration_report([[2, 2, Q_ONE]], [5, 0, 0], [0.0] * 5)
    # the accumulator adds integers and float64 sums
    acc = CalibrationAccumulator(1)
    for _ in range(3):
        acc.update(SimpleNamespace(hist=torch.tensor([[10, 7, 9 * Q_ONE]]), tail=torch.tensor([10, 0, 0]), sums=torch.full((5,), 0.1)))
    rep = acc.result()
    assert rep["pixels"] == 30 and rep["ece"] == 0.2 and abs(rep["nll"] - 0.1 * 3 / 30) < 1e-9
    with pytest.raises(ValueError, match="1 bins"):
        acc.update(SimpleNamespace(hist=torch.zeros((2, 3), dtype=torch.int64), tail=torch.zeros(3), sums=torch.zeros(5)))


# ------------------------------------------------------------------------------------------ fit_temperature with the oracle as the kernel
class _Stub:
    """Stands in for ops.seg_calib: the oracle's float64 (NLL, G, H) as the five sums, and the valid-pixel count."""

    def __init__(self):
        self.cache, self.calls = {}, []

    def __call__(self, z, u, labels, *, inv_temperature, want_pred):
        assert want_pred is False
        key = id(z)
        if key not in self.cache:
            g = math.isqrt(z.shape[1])
            self.cache[key] = CO.Calib(z.numpy(), labels.numpy(), g, u)
        cal = self.cache[key]
        nll, G, H = cal.newton(inv_temperature)
        self.calls.append(inv_temperature)
        return SimpleNamespace(sums=torch.tensor([nll, 0.0, G, H, 0.0], dtype=torch.float64), tail=torch.tensor([cal.nv, 0, 0]))


def _calibrated_batches(k, seed=0, n=2, g=3, u=4, C=4):
    """Labels drawn from the softmax of a random field's upsampled logits; the batch's logits are k times the field: T = k is well
    calibrated up to sampling noise."""
    import _segloss_oracle as SO
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        z = rng.standard_normal((2, g * g, C)).astype(np.float32)
        l = SO.upsample(z, g, u)
        p = np.exp(l - l.max(-1, keepdims=True))
        p /= p.sum(-1, keepdims=True)
        y = (p.cumsum(-1) < rng.random(p.shape[:-1] + (1,))).sum(-1).clip(0, C - 1).astype(np.uint8)
        out.append((torch.from_numpy((k * z).astype(np.float32)), torch.from_numpy(y)))
    return out


@pytest.mark.parametrize("k", [3.0, 0.5])
def test_fit_temperature_converges_inside_the_bracket(k):
    from dinox.segment import fit_temperature
    batches, stub = _calibrated_batches(k), _Stub()
    fit = fit_temperature(batches, 4, calib=stub)
    s_star = CO.root_of_g([stub.cache[id(z)] for z, _ in batches])
    assert fit["converged"] and 0.05 < fit["temperature"] < 20.0 and 1 <= fit["iterations"] <= 30
    assert abs(math.log(1.0 / fit["temperature"]) - math.log(s_star)) <= 1e-4
    assert abs(math.log(fit["temperature"] / k)) < 0.5          # sampling noise only: the labels came from the field at T = k
    assert fit["nll_after"] <= fit["nll_before"]
    assert stub.calls[0] == 1.0 and len(stub.calls) == 2 * (fit["iterations"] + 1)
    assert abs(stub.calls[-1] - 1.0 / fit["temperature"]) <= 1e-12 * stub.calls[-1]      # nll_after was measured at the returned temperature


def test_fit_temperature_bisects_when_newton_overshoots():
    """Logits at half their calibrated scale (the root lies near s = 2, so G(1) < 0) and a stub that understates the curvature wherever
    G < 0 so that the denominator s G + s^2 H is barely positive: the Newton step from s = 1 is enormous, leaves the bracket, and the
    midpoint is taken instead; the fit still lands on the root of G."""
    from dinox.segment import fit_temperature
    batches, inner = _calibrated_batches(0.5, seed=1, n=1), _Stub()

    def flat(z, u, labels, *, inv_temperature, want_pred):
        r = inner(z, u, labels, inv_temperature=inv_temperature, want_pred=want_pred)
        if r.sums[2] < 0:
            r.sums[3] = (1e-9 - r.sums[2]) / inv_temperature
        return r

    fit = fit_temperature(batches, 4, calib=flat, max_iter=60)
    thetas = [math.log(s) for s in inner.calls]
    a, b = -math.log(20.0), math.log(20.0)
    assert thetas[0] == 0.0 and abs(thetas[1] - 0.5 * (0.0 + b)) < 1e-12      # G(1) < 0: the lower end moves to 0, then the midpoint
    assert all(a <= t <= b for t in thetas)
    s_star = CO.root_of_g([inner.cache[id(z)] for z, _ in batches])
    assert fit["converged"] and abs(math.log(1.0 / fit["temperature"]) - math.log(s_star)) <= 1e-4
    # a denominator <= 0 takes the midpoint too
    def concave(z, u, labels, *, inv_temperature, want_pred):
        r = inner(z, u, labels, inv_temperature=inv_temperature, want_pred=want_pred)
        r.sums[3] = -abs(r.sums[2]) / inv_temperature - 1.0
        return r
    fit = fit_temperature(batches, 4, calib=concave, max_iter=60)
    assert fit["converged"] and abs(math.log(1.0 / fit["temperature"]) - math.log(s_star)) <= 1e-4


def test_fit_temperature_without_a_valid_pixel():
    from dinox.segment import fit_temperature
    z = torch.zeros((1, 4, 3))
    y = torch.full((1, 4, 4), 255, dtype=torch.uint8)
    fit = fit_temperature([(z, y)], 2, calib=_Stub())
    assert fit["temperature"] == 1.0 and fit["converged"] is False and fit["iterations"] == 0
    with pytest.raises(ValueError, match="lo < hi"):
        fit_temperature([(z, y)], 2, lo=2.0, hi=1.0, calib=_Stub())


# ------------------------------------------------------------------------------------------ the C entries refuse on the host
def test_argument_refusal_without_a_gpu():
    from dinox import _lib
    lib, f = _lib.lib, ctypes.c_float
    z, y, out, hist, sums, ws = (ctypes.c_void_p(0x1000 * (i + 1)) for i in range(6))        # never dereferenced: refused before any launch
    good = dict(B=2, g=3, u=4, C=5, NB=15)

    def call(s=1.0, y=y, hist=hist, sums=sums, ws=ws, pred=out, **kw):
        a = dict(good, **kw)
        return lib.dinox_seg_calib(z, y, f(s), pred, None, None, hist, sums, ws, a["B"], a["g"], a["u"], a["C"], a["NB"], None)

    assert lib.dinox_seg_calib_ws_bytes(2, 3, 4, 5, 15) > 0
    for nb in (0, 65, -1):
        assert call(NB=nb) == -1 and "NB" in _lib.last_error()
        assert lib.dinox_seg_calib_ws_bytes(2, 3, 4, 5, nb) == 0
    for s in (0.0, -1.0, float("inf"), float("nan")):
        assert call(s=s) == -1 and "inv_temperature" in _lib.last_error()
    assert call(hist=None) == -1 and "all four or none" in _lib.last_error()               # y without hist
    assert call(sums=None) == -1 and call(ws=None) == -1
    assert call(y=None) == -1 and "all four or none" in _lib.last_error()                  # hist without y
    assert call(y=None, hist=None, sums=None, ws=None, pred=None) == -1 and "nothing to compute" in _lib.last_error()
    assert lib.dinox_seg_calib(None, y, f(1.0), out, None, None, hist, sums, ws, 2, 3, 4, 5, 15, None) == -1 and "null" in _lib.last_error()
    for kw, word in ((dict(C=1), "C=1"), (dict(u=33), "u=33"), (dict(B=0), "B=0"), (dict(g=0), "g=0")):
        assert call(**kw) != 0 and word in _lib.last_error()
        a = dict(good, **kw)
        assert lib.dinox_seg_calib_ws_bytes(a["B"], a["g"], a["u"], a["C"], a["NB"]) == 0
    assert call(C=65) == -2 and lib.dinox_seg_calib_ws_bytes(2, 3, 4, 65, 15) == 0
    assert lib.dinox_version() == 3


def test_ops_refuses_before_the_device():
    from dinox import ops
    z = torch.zeros((1, 4, 3))
    with pytest.raises(ValueError, match="bins"):
        ops.seg_calib(z, 2, bins=0)
    with pytest.raises(ValueError, match="bins"):
        ops.seg_calib(z, 2, bins=65)
    for s in (0.0, -2.0, float("inf"), float("nan"), 1e-60):
        with pytest.raises(ValueError, match="inv_temperature"):
            ops.seg_calib(z, 2, inv_temperature=s)
    with pytest.raises(ValueError, match="nothing to compute"):
        ops.seg_calib(z, 2, want_pred=False)
    with pytest.raises(ValueError, match="do not have side"):
        ops.seg_calib(z, 2, torch.zeros((1, 8, 8), dtype=torch.uint8))
    with pytest.raises(ValueError, match=r"C must lie in \[2, 64\]"):
        ops.seg_calib(torch.zeros((1, 4, 65)), 2)


# ------------------------------------------------------------------------------------------ scripts
def _script(name):
    if name in sys.modules:
        return sys.modules[name]
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "dino-x_amd", "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def test_evaluate_segmentation_flags(capsys):
    es = _script("evaluate_segmentation")
    ap = es.build_parser()
    base = ["--backbone", "b", "--segmenter", "s", "--synthetic", "8"]
    a = ap.parse_args(base)
    assert (a.calibration, a.calibration_bins, a.temperature, a.fit_temperature, a.write_temperature, a.calibration_cache_gib) == \
        (False, 15, None, False, False, 4.0)
    es.check_args(ap, a)
    a = ap.parse_args(base + ["--calibration", "--calibration-bins", "10", "--temperature", "1.5"])
    assert a.calibration and a.calibration_bins == 10 and a.temperature == 1.5
    es.check_args(ap, a)
    es.check_args(ap, ap.parse_args(base + ["--fit-temperature", "--write-temperature"]))
    for bad, word in ((["--write-temperature"], "--write-temperature needs --fit-temperature"), (["--calibration-bins", "0"], "--calibration-bins"),
                      (["--calibration-bins", "65"], "--calibration-bins"), (["--temperature", "0"], "--temperature"),
                      (["--calibration-cache-gib", "0"], "--calibration-cache-gib")):
        with pytest.raises(SystemExit) as e:
            es.check_args(ap, ap.parse_args(base + bad))
        assert e.value.code == 2 and word in capsys.readouterr().err
    help_text = "".join(ap.format_help().split())             # (argparse may wrap inside a hyphenated flag)
    assert "--keep-largestand--min-component-mm2donotaffectit" in help_text


def test_segment_volume_flags(capsys):
    sv = _script("segment_volume")
    ap = sv.build_parser()
    base = ["--backbone", "b", "--segmenter", "s", "--volume", "v.npy", "--spacing", "1", "1", "1", "--out", "o.npy"]
    a = ap.parse_args(base)
    assert a.confidence_out is None and a.entropy_out is None
    a = ap.parse_args(base + ["--confidence-out", "c.npy", "--entropy-out", "e.npy"])
    sv.check_args(ap, a)
    assert str(a.confidence_out) == "c.npy" and str(a.entropy_out) == "e.npy"
    sv.check_args(ap, ap.parse_args(base + ["--tiled", "--confidence-out", "c.npy"]))
    with pytest.raises(SystemExit) as e:
        sv.check_args(ap, ap.parse_args(base + ["--tiled", "--entropy-out", "e.npy"]))
    assert e.value.code == 2 and "--entropy-out: not with --tiled" in capsys.readouterr().err
    assert "near-ties" in "".join(ap.format_help().split())


def test_finetune_segmentation_flag():
    fs = _script("finetune_segmentation")
    base = ["--backbone", "b", "--synthetic", "8", "--output", "o"]
    assert fs.parse_cli(base).fit_temperature is False
    assert fs.parse_cli(base + ["--fit-temperature"]).fit_temperature is True
    assert {s for a in fs.build_calibration_parser()._actions for s in a.option_strings} == {"--fit-temperature"}
