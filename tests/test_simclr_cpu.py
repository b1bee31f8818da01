"""SimCLR objective, host side: the float64 NT-Xent oracle against what the reference's SimCLRLoss + autograd recorded
(tests/golden/simclr_loss.npz), the oracle's invariances, the C ABI surface and the CLI's argument checks.  No kernel is launched."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden

import _ntxent_oracle as NX

CASES = ["b3", "b33", "b130", "adv"]


@pytest.fixture(scope="module")
def gold():
    return load_golden("simclr_loss.npz")


def row_err(got, want):
    """max over rows of (max-abs error of the row / max-abs of the reference row); a zero reference row must be matched exactly."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = np.abs(want).max(1)
    err = np.abs(got - want).max(1)
    assert (err[scale == 0] == 0).all()
    return float((err[scale > 0] / scale[scale > 0]).max())


@pytest.mark.parametrize("tag", CASES)
def test_oracle_matches_reference_fixture(gold, tag):
    """Loss within rel 1e-6 and every gradient row within 2e-6 of the row's max-abs: the reference ran in fp32, the oracle in fp64
    (measured when the fixture was made: 4e-8 and 8e-7, the latter on the rows below eps whose gradients are ~7e11)."""
    assert float(gold["temperature"]) == 0.1 and list(gold["cases"]) == CASES
    loss, dz1, dz2 = NX.simclr(gold[f"{tag}_z1"], gold[f"{tag}_z2"], 0.1)
    want = float(gold[f"{tag}_loss"])
    e1, e2 = row_err(dz1, gold[f"{tag}_dz1"]), row_err(dz2, gold[f"{tag}_dz2"])
    print(f"{tag}: loss rel err {abs(loss - want) / abs(want):.2e}, worst gradient row {max(e1, e2):.2e}")
    assert abs(loss - want) <= 1e-6 * abs(want)
    assert np.isfinite(dz1).all() and np.isfinite(dz2).all()
    assert max(e1, e2) <= 2e-6


def test_adversarial_fixture_holds_its_edge_cases(gold):
    z1, z2, eps = gold["adv_z1"].astype(np.float64), gold["adv_z2"].astype(np.float64), 1e-12
    n1, n2 = np.linalg.norm(z1, axis=1), np.linalg.norm(z2, axis=1)
    assert (z1[0] == z2[0]).all()                                    # duplicated pair
    assert 0 < n1[1] < eps and n1[2] > 1e3 and n2[6] == 0            # below eps, long, all-zero
    cos = lambda a, b: float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)))
    assert cos(z1[3], z1[4]) > 1 - 1e-6 and cos(z1[5], z2[5]) < -1 + 1e-6
    assert np.abs(gold["adv_dz1"][1]).max() > 1e10                   # dz = dzh / eps on the clamped row


def test_oracle_is_invariant_under_view_swap_and_row_scaling(gold):
    z1, z2 = gold["b33_z1"].astype(np.float64), gold["b33_z2"].astype(np.float64)
    loss, dz1, dz2 = NX.simclr(z1, z2)
    loss_s, dz2_s, dz1_s = NX.simclr(z2, z1)
    assert loss_s == pytest.approx(loss, rel=1e-13)
    assert np.allclose(dz1_s, dz1, rtol=1e-10, atol=1e-18) and np.allclose(dz2_s, dz2, rtol=1e-10, atol=1e-18)
    c = np.random.default_rng(0).uniform(0.01, 100.0, size=(33, 1))
    loss_c, dz1_c, _ = NX.simclr(z1 * c, z2)
    assert loss_c == pytest.approx(loss, rel=1e-12)
    assert np.allclose(dz1_c * c, dz1, rtol=1e-9, atol=1e-18)        # the loss depends on the direction only: dz scales by 1/c
    # ... and only rows at or above eps: scaling the clamped row of the adversarial case DOES change the loss
    a1, a2 = gold["adv_z1"].astype(np.float64), gold["adv_z2"].astype(np.float64)
    b1 = a1.copy()
    b1[1] *= 1e3
    assert abs(NX.simclr(b1, a2)[0] - NX.simclr(a1, a2)[0]) > 1e-8


def test_oracle_gradient_is_the_derivative_of_its_loss():
    rng = np.random.default_rng(3)
    z = rng.normal(size=(6, 5))
    loss, dz = NX.ntxent(z, 0.1)
    for (i, d) in [(0, 0), (2, 3), (5, 4)]:
        h = 1e-6
        zp, zm = z.copy(), z.copy()
        zp[i, d] += h
        zm[i, d] -= h
        assert (NX.ntxent(zp)[0] - NX.ntxent(zm)[0]) / (2 * h) == pytest.approx(dz[i, d], rel=1e-6, abs=1e-9)
    with pytest.raises(ValueError):
        NX.ntxent(z[:5])


def test_step_fixture_is_complete(golden):
    g = golden("simclr_step_tiny.npz")
    names = list(g["param_order"])
    assert 0.0 <= float(g["small_grad_share"]) <= 0.10
    assert g["batch0"].shape == (8, 3, 28, 28) and g["spacing0"].shape == (8, 3) and len(g["losses"]) == 3
    for step in range(3):
        assert {k[len(f"grad{step}/"):] for k in g if k.startswith(f"grad{step}/")} == set(names)
    assert {k[5:] for k in g if k.startswith("init/")} == {k[9:] for k in g if k.startswith("student3/")} >= set(names)
    small = total = 0
    for n in names:
        m = np.zeros(g[f"grad0/{n}"].shape, bool)
        for step in range(3):
            m |= np.abs(g[f"grad{step}/{n}"]) < 1e-6
        small, total = small + int(m.sum()), total + m.size
    assert small / total == pytest.approx(float(g["small_grad_share"]), abs=1e-12)


NEW_CALLS = {"dinox_ntxent_rows": 8, "dinox_ntxent_coeff": 9, "dinox_normalize_bwd": 8}


def test_header_and_ctypes_table_declare_the_new_calls():
    src = open(os.path.join(ROOT, "include", "dinox.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    from dinox import _lib
    for name, nargs in NEW_CALLS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;{]*?)\)\s*;", src, flags=re.S)
        assert m, f"{name} is not declared in include/dinox.h"
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == nargs and args[-1] == "void* stream"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert hasattr(_lib.lib, name)
    assert _lib.lib.dinox_version() == 3


def test_abi_rejects_bad_arguments_before_any_launch():
    """Odd M, M < 2 and null pointers come back as an error code with a message (the checks run on the host, ahead of the launch:
    the pointers below are never dereferenced)."""
    import ctypes as C
    from dinox import _lib
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    for M in (3, 1, 0):
        assert _lib.lib.dinox_ntxent_rows(p, 8, M, 10.0, p, p, p, None) == -1 and "M=" in _lib.last_error()
        assert _lib.lib.dinox_ntxent_coeff(p, 8, p, M, 10.0, 1.0, p + 128, 8, None) == -1 and "M=" in _lib.last_error()
    assert _lib.lib.dinox_ntxent_rows(None, 8, 4, 10.0, p, p, p, None) == -1 and "null" in _lib.last_error()
    assert _lib.lib.dinox_ntxent_coeff(p, 8, None, 4, 10.0, 1.0, p + 128, 8, None) == -1 and "null" in _lib.last_error()
    assert _lib.lib.dinox_ntxent_coeff(p, 8, p, 4, 10.0, 1.0, p, 8, None) == -1 and "alias" in _lib.last_error()
    assert _lib.lib.dinox_ntxent_rows(p, 3, 4, 10.0, p, p, p, None) == -1 and "lds" in _lib.last_error()
    assert _lib.lib.dinox_normalize_bwd(p, p, None, p, 4, 8, 1e-12, None) == -1 and "null" in _lib.last_error()
    assert _lib.lib.dinox_normalize_bwd(p, p, p, p, 0, 8, 1e-12, None) == -1 and "V=" in _lib.last_error()


def test_ops_reject_cpu_tensors_and_odd_row_counts():
    import torch
    from dinox import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ntxent_fwd(torch.randn(4, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.simclr_loss(torch.randn(2, 8), torch.randn(2, 8))
    for name in ("ntxent_fwd", "ntxent_bwd", "NTXentFn", "simclr_loss"):
        assert hasattr(ops, name)


def test_engine_hyperparameters_gain_the_simclr_fields():
    from dinox.engine import StepHyperParams
    hp = StepHyperParams()
    assert hp.loss_type == "dino" and hp.simclr_temp == 0.1


def test_cli_rejects_simclr_with_local_crops_and_mae_without_a_device(cli, monkeypatch):
    """Both exits come from the argument check at the top of main(): nothing may reach the process group or the device."""
    def boom(*a, **k):
        raise AssertionError("the argument check must run before any device work")
    monkeypatch.setattr(cli, "init_process_group", boom)
    monkeypatch.setattr(cli, "detect_hardware", boom)
    with pytest.raises(SystemExit, match="simclr.*--local-crops"):
        cli.main(["--loss-type", "simclr", "--local-crops", "2", "--gpu-views", "--synthetic", "8"])
    with pytest.raises(SystemExit, match="mae is not wired"):
        cli.main(["--loss-type", "mae", "--synthetic", "8"])
    args = cli.build_parser().parse_args(["--loss-type", "simclr"])
    cli.check_loss_type(args, world=1)
    with pytest.raises(SystemExit, match="one GPU only"):
        cli.check_loss_type(args, world=2)
