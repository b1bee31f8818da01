"""Sinkhorn-Knopp teacher centring, host side: the centre identity (softmax((t - sk_center) / tau) is the published loop's Q), the
marginals of the loop, an fp32 NumPy evaluation of the recurrence against the bounds tests/test_sinkhorn_gpu.py holds the kernels to,
and the surfaces -- command line, hyper-parameters, C header and library exports.  No kernel is launched."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import _sinkhorn_oracle as SK

F32 = np.float32
SHAPES = [(6, 5), (2, 64), (130, 257)]


def inside(got, ref, bound, what):
    ratio = np.abs(np.asarray(got, np.float64) - ref) / bound
    assert np.isfinite(np.asarray(got, np.float64)).all() and ratio.max() <= 1.0, f"{what}: fp32 evaluation at {ratio.max():.3f} of the bound"
    return float(ratio.max())


def moderate(R, K, seed):
    """Logits of a unit or so: exp(t / tau) stays far inside float64 at tau = 0.04 (|z| < 200)."""
    return np.random.default_rng(seed).standard_normal((R, K)).astype(np.float32)


# ------------------------------------------------------------------------------------------ the identity
@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("tt", [0.04, 0.07])
@pytest.mark.parametrize("R,K", SHAPES)
def test_center_identity_against_the_published_loop(R, K, tt, iters):
    t = moderate(R, K, R + K)
    q = SK.sk_literal(t, tt, iters)
    assert np.abs(q.sum(1) - 1).max() < 1e-12                               # one assignment per sample
    p = SK.targets(t, SK.sk_center(t, tt, iters), tt)
    assert np.abs(p - q).max() <= 1e-12, np.abs(p - q).max()


@pytest.mark.parametrize("regime", ["onehot", "wide"])
def test_identity_holds_where_float64_overflows(regime):
    """The logit regimes of the GPU tests leave float64 in the linear domain (onehot: z up to 1750); the same loop in long double
    (x87: exponents to 2^16384) stays finite and still equals the log-domain statement."""
    if np.finfo(np.longdouble).maxexp <= np.finfo(np.float64).maxexp:
        pytest.skip("long double is float64 on this host")
    t, tt = SK.sk_inputs(regime, 7, 257, seed=3)
    q = SK.sk_literal(t, tt, 3, dt=np.longdouble)
    assert np.isfinite(q).all()
    p = SK.targets(t, SK.sk_center(t, tt, 3), tt)
    assert np.abs(p - q.astype(np.float64)).max() <= 1e-9


@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("R,K", SHAPES)
def test_prototype_marginals_before_the_closing_row_normalisation(R, K, iters):
    """After the last prototype pass, before any further row normalisation: Q' = exp(z + a_{n-1} + b_n) has columns that sum to 1, i.e.
    the published Q (which carries 1/K per prototype and B per sample) has column sums * K / R equal to 1 at that point."""
    t = moderate(R, K, 3 * R + K)
    tt = 0.04
    trace = []
    c = SK.sk_center(t, tt, iters, trace=trace)
    last = trace[-1]                                                        # the last column pass: x = z + a_{n-1}
    q = np.exp(last["x"] + (-c / SK.f32(tt))[None, :]) * (R / K)            # the published scaling: every prototype holds R / K samples
    assert np.abs(q.sum(0) * K / R - 1).max() < 1e-12
    # the published loop, stopped at the same place
    Q = np.exp(t.astype(np.float64) / SK.f32(tt)).T
    Q /= Q.sum()
    for n in range(iters):
        if n:
            Q /= Q.sum(0, keepdims=True); Q /= R
        Q /= Q.sum(1, keepdims=True); Q /= K
    assert np.abs(Q.sum(1) * K - 1).max() < 1e-12
    assert np.abs(Q.T * K - q * K / R).max() <= 1e-12                       # the same matrix, in the loop's scaling (1/K per prototype)


# ------------------------------------------------------------------------------------------ an fp32 evaluation stays inside the bounds
@pytest.mark.parametrize("regime", ["normal", "onehot", "wide"])
@pytest.mark.parametrize("R,K", [(1, 8), (2, 5), (6, 64), (7, 257), (33, 4100), (130, 1028)])
def test_fp32_passes_stay_inside_their_bounds(regime, R, K):
    t, tt = SK.sk_inputs(regime, R, K, seed=R + K)
    inv = SK.inv_temp(tt)
    r = np.random.default_rng(K)
    for a in (None, (-500 * r.random(R)).astype(F32)):
        ref, parts = SK.col_pass(t, a, inv)
        inside(SK.col_pass(t, a, inv, dt=F32)[0], ref, SK.bound_pass(parts), "column pass")
    for b in (None, (-500 * r.random(K)).astype(F32)):
        ref, parts = SK.row_pass(t, b, inv)
        inside(SK.row_pass(t, b, inv, dt=F32)[0], ref, SK.bound_pass(parts), "row pass")


@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("regime", ["normal", "onehot", "wide"])
@pytest.mark.parametrize("R,K", [(2, 5), (7, 257), (130, 1028)])
def test_fp32_recurrence_stays_inside_the_carried_bound(regime, R, K, iters):
    t, tt = SK.sk_inputs(regime, R, K, seed=R + K)
    c, bound = SK.bound_center(t, tt, iters)
    lo = SK.sk_center(t, tt, iters, dt=F32)
    assert lo.dtype == F32
    inside(lo, c, bound, "centre")
    assert (bound < 1e-3 * max(1.0, float(np.abs(c).max()))).all()          # and the bound says something: 1e-3 of the centre at the most


def test_wide_regime_underflows_and_onehot_is_onehot():
    t, tt = SK.sk_inputs("wide", 33, 4100, seed=1)
    _, parts = SK.col_pass(t, None, SK.inv_temp(tt))
    assert (np.exp((parts["x"] - parts["m"]).astype(F32)) == 0).mean() > 0.5
    t, tt = SK.sk_inputs("onehot", 6, 64, seed=1)
    assert (SK.targets(t, SK.dino_inputs("onehot", 6, 6, 64, 1)[2], tt).max(1) > 1 - 1e-6).all()      # (against the centre it was drawn around)


# ------------------------------------------------------------------------------------------ surfaces
def test_parser_flags_and_refusals(cli):
    d = cli.parse_cli([])
    assert d.centering == "ema" and d.sk_iters == 3
    a = cli.parse_cli(["--centering", "sinkhorn", "--sk-iters", "2", "--batch-size", "8"])
    assert a.centering == "sinkhorn" and a.sk_iters == 2 and a.batch_size == 8
    with pytest.raises(SystemExit):
        cli.parse_cli(["--centering", "mean"])
    base = ["--centering", "sinkhorn", "--mae-decoder", "64x1x2"]
    cli.check_loss_type(cli.parse_cli(base))                                # dino: fine
    for lt in ("simclr", "mae"):
        with pytest.raises(SystemExit, match="--centering sinkhorn"):
            cli.check_loss_type(cli.parse_cli(base + ["--loss-type", lt]))
        cli.check_loss_type(cli.parse_cli(["--mae-decoder", "64x1x2", "--loss-type", lt]))      # ... and fine with the EMA centre
    with pytest.raises(SystemExit, match="--sk-iters"):
        cli.check_loss_type(cli.parse_cli(["--centering", "sinkhorn", "--sk-iters", "0"]))


def test_saved_config_names_the_extension_only_when_it_is_on(cli):
    cfg = cli.TrainingConfig(model=cli.MODEL_CONFIGS["vit-small"])
    from dataclasses import asdict
    from dinox.engine import StepHyperParams
    for default in (None, cli.parse_cli([]), StepHyperParams()):
        assert cli.config_dict(cfg, default) == asdict(cfg)                 # default run: the bytes it always wrote
    d = cli.config_dict(cfg, cli.parse_cli(["--centering", "sinkhorn", "--sk-iters", "2"]))
    assert d["centering"] == "sinkhorn" and d["sk_iters"] == 2 and d["teacher_temp"] == 0.04
    d = cli.config_dict(cfg, StepHyperParams(sk_iters=5))                   # (a non-default count is recorded with the EMA centre too)
    assert d["centering"] == "ema" and d["sk_iters"] == 5


def test_hyper_parameter_defaults():
    from dinox.engine import StepHyperParams
    hp = StepHyperParams()
    assert hp.centering == "ema" and hp.sk_iters == 3


def test_header_declares_and_library_exports_the_entries():
    from dinox import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dinox.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("dinox_sk_col_lse", "dinox_sk_row_lse", "dinox_sk_center", "dinox_sk_ws_floats"):
        assert re.search(r"\b" + name + r"\s*\(", src), f"{name} not declared in dinox.h"
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert _lib.lib.dinox_sk_ws_floats(512, 8192) == 2 * 16 * 8192 + 8192 + 512
    assert _lib.lib.dinox_sk_ws_floats(33, 5) == 2 * 2 * 5 + 5 + 33


def test_entries_reject_bad_arguments_without_a_launch():
    """Host-side validation: the library's argument error, dinox_last_error set, nothing launched (safe without a GPU)."""
    from dinox import _lib
    L = _lib.lib
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    for n_iters, R, K, word in ((0, 4, 4, "n_iters"), (3, 0, 4, "R=0"), (3, 4, 0, "K=0"), (-1, 4, 4, "n_iters")):
        assert L.dinox_sk_center(p, 0.04, n_iters, p, p, R, K, None) == -1 and word in _lib.last_error(), _lib.last_error()
    assert L.dinox_sk_center(p, 0.0, 3, p, p, 4, 4, None) == -1 and "teacher_temp" in _lib.last_error()
    assert L.dinox_sk_center(None, 0.04, 3, p, p, 4, 4, None) == -1 and "null" in _lib.last_error()
    assert L.dinox_sk_col_lse(p, None, 1.0, 1.0, p, p, 0, 4, None) == -1 and L.dinox_sk_col_lse(p, None, 1.0, 1.0, p, None, 4, 4, None) == -1
    assert L.dinox_sk_row_lse(p, None, 1.0, 1.0, p, 4, 0, None) == -1 and L.dinox_sk_row_lse(p, None, 1.0, 1.0, None, 4, 4, None) == -1
    assert L.dinox_sk_ws_floats(0, 4) == 0


def test_engine_refuses_what_it_does_not_run():
    """The constructor's refusals come before it touches a module or a device."""
    from dinox.engine import StepHyperParams, TrainEngine
    for hp, word in ((StepHyperParams(centering="mean"), "centering"), (StepHyperParams(centering="sinkhorn", sk_iters=0), "sk_iters"),
                     (StepHyperParams(centering="sinkhorn", loss_type="simclr"), "sinkhorn"),
                     (StepHyperParams(centering="sinkhorn", loss_type="mae"), "sinkhorn")):
        with pytest.raises(ValueError, match=word):
            TrainEngine(None, None, 16, hp)
