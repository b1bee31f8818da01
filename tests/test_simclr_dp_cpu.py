"""Data-parallel SimCLR without a device: the algebra of the sharded NT-Xent formulas (tests/_ntxent_dp_oracle.py) against the float64
oracle of the global batch, the command line (--simclr-negatives), the hyper-parameter and the C-ABI surface of the rectangular entry
points."""
import ctypes as C
import json
import os
from dataclasses import asdict

import numpy as np
import pytest

from conftest import ROOT

import _ntxent_dp_oracle as DP
import _ntxent_oracle as NX


# ------------------------------------------------------------------------------------------ the algebra
@pytest.mark.parametrize("world,Bl,D", [(2, 3, 5), (3, 17, 64), (4, 1, 8), (1, 33, 64)])
def test_sharded_formulas_give_the_global_loss_and_world_times_its_gradient(world, Bl, D):
    """Every rank's rectangular lse / W / normalize_bwd, concatenated, is the NT-Xent of the permuted global batch [z1 of all ranks; z2
    of all ranks]: the loss as it is, the gradient after dividing by ``world`` (the gradient convention).  1e-12 relative: both sides
    are float64 and differ in summation order only."""
    rng = np.random.default_rng(1000 * world + Bl)
    B = world * Bl
    z1, z2 = 2.0 * rng.standard_normal((B, D)), 2.0 * rng.standard_normal((B, D))
    loss, dz, lse = DP.ntxent_sharded(DP.split(z1, z2, world), 0.1)
    want_loss, want_dz = NX.ntxent(np.concatenate([z1, z2], 0), 0.1)
    got_dz = DP.unsplit(dz) / world
    assert got_dz.shape == want_dz.shape == (2 * B, D)
    assert abs(loss - want_loss) <= 1e-12 * abs(want_loss)
    err = np.abs(got_dz - want_dz).max()
    print(f"world {world}, Bl {Bl}, D {D}: loss rel err {abs(loss - want_loss) / abs(want_loss):.1e}, gradient err {err / np.abs(want_dz).max():.1e}")
    assert err <= 1e-12 * np.abs(want_dz).max()
    assert all(l.shape == (2 * Bl,) for l in lse)


def test_split_and_unsplit_are_inverse_permutations():
    z1, z2 = np.arange(12.0).reshape(6, 2), 100 + np.arange(12.0).reshape(6, 2)
    parts = DP.split(z1, z2, 3)
    assert [p.shape for p in parts] == [(4, 2)] * 3 and np.array_equal(parts[1], np.concatenate([z1[2:4], z2[2:4]], 0))
    assert np.array_equal(DP.unsplit(parts), np.concatenate([z1, z2], 0))


def test_sharded_oracle_handles_the_adversarial_rows():
    """The adversarial fixture (a duplicated pair, a row below eps, parallel rows across the two ranks, an all-zero row) in two shards."""
    from conftest import load_golden
    g = load_golden("simclr_loss.npz")
    z1, z2 = g["adv_z1"].astype(np.float64), g["adv_z2"].astype(np.float64)
    loss, dz, _ = DP.ntxent_sharded(DP.split(z1, z2, 2), 0.1)
    want_loss, want_dz = NX.ntxent(np.concatenate([z1, z2], 0), 0.1)
    got = DP.unsplit(dz) / 2
    assert abs(loss - want_loss) <= 1e-12 * abs(want_loss) and np.isfinite(got).all()
    scale = np.abs(want_dz).max(1)
    assert (np.abs(got - want_dz).max(1) <= 1e-9 * scale).all()        # (rows at 1e11 next to rows at 1e-3: per row, cancellation included)


# ------------------------------------------------------------------------------------------ the command line
def test_cli_accepts_global_negatives_on_several_ranks(cli):
    args = cli.parse_cli(["--loss-type", "simclr", "--simclr-negatives", "global"])
    assert args.simclr_negatives == "global"
    cli.check_loss_type(args, world=1)
    cli.check_loss_type(args, world=2)
    cli.check_loss_type(args, world=8)


def test_cli_local_negatives_still_exit_on_several_ranks(cli):
    for argv in (["--loss-type", "simclr"], ["--loss-type", "simclr", "--simclr-negatives", "local"]):
        args = cli.parse_cli(argv)
        assert args.simclr_negatives == "local"
        cli.check_loss_type(args, world=1)
        with pytest.raises(SystemExit, match="one GPU only.*--simclr-negatives"):
            cli.check_loss_type(args, world=2)


def test_cli_flag_belongs_to_simclr(cli):
    with pytest.raises(SystemExit, match="--simclr-negatives global belongs to --loss-type simclr"):
        cli.check_loss_type(cli.parse_cli(["--loss-type", "dino", "--simclr-negatives", "global"]))
    with pytest.raises(SystemExit, match="--simclr-negatives"):
        cli.check_loss_type(cli.parse_cli(["--simclr-negatives", "global", "--loss-type", "mae", "--mae-decoder", "64x1x2"]))
    cli.check_loss_type(cli.parse_cli(["--loss-type", "dino", "--simclr-negatives", "local"]))       # the default, spelled out
    with pytest.raises(SystemExit):
        cli.parse_cli(["--loss-type", "simclr", "--simclr-negatives", "everything"])
    assert "--simclr-negatives" in cli.__doc__


def test_saved_config_names_the_negatives_only_when_global(cli):
    from dinox.engine import StepHyperParams
    cfg = cli.TrainingConfig(model=cli.MODEL_CONFIGS["vit-small"], loss_type="simclr", created_at="2026-01-01 00:00:00 UTC")
    plain = json.dumps(asdict(cfg), indent=2) + "\n"
    for default in (None, cli.parse_cli(["--loss-type", "simclr"]), StepHyperParams(loss_type="simclr")):
        assert json.dumps(cli.config_dict(cfg, default), indent=2) + "\n" == plain          # a default run: the bytes it always wrote
    for on in (cli.parse_cli(["--loss-type", "simclr", "--simclr-negatives", "global"]),
               StepHyperParams(loss_type="simclr", simclr_negatives="global")):
        d = cli.config_dict(cfg, on)
        assert d["simclr_negatives"] == "global" and "centering" not in d
        d.pop("simclr_negatives")
        assert d == asdict(cfg)


# ------------------------------------------------------------------------------------------ the engine's hyper-parameter
def test_hyper_parameter_default_and_bad_value():
    import torch
    import zoo.arch as arch
    from dinox.engine import StepHyperParams, TrainEngine
    assert StepHyperParams().simclr_negatives == "local"
    kw = dict(img_size=28, patch=14, dim=32, depth=1, heads=2, num_registers=0, scale_aware=False)
    torch.manual_seed(0)
    student, teacher = arch.DinoStudentTeacher(arch.PatchViT(**kw), 48), arch.DinoStudentTeacher(arch.PatchViT(**kw), 48)
    with pytest.raises(ValueError, match="simclr_negatives must be 'local' or 'global'"):
        TrainEngine(student, teacher, 48, StepHyperParams(loss_type="simclr", simclr_negatives="all"))
    with pytest.raises(ValueError, match="simclr_negatives='global' belongs to loss_type='simclr'"):
        TrainEngine(student, teacher, 48, StepHyperParams(simclr_negatives="global"))
    eng = TrainEngine(student, teacher, 48, StepHyperParams(loss_type="simclr", simclr_negatives="global"))       # one rank: nothing to gather
    assert eng._ntxent_group is None


# ------------------------------------------------------------------------------------------ the C-ABI surface
NAMES = ("dinox_ntxent_rows_rect", "dinox_ntxent_coeff_rect")


def test_new_entry_points_are_declared_exported_and_bound():
    from dinox import _lib
    header = open(os.path.join(ROOT, "include", "dinox.h")).read()
    ntxent_hip = open(os.path.join(ROOT, "dino-x_amd", "csrc", "ntxent.hip")).read()
    exported = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert f"int {name}(" in header and name in _lib.SIGNATURES and hasattr(exported, name)
        assert f'extern "C" int {name}(' in ntxent_hip
    assert len(_lib.SIGNATURES["dinox_ntxent_rows_rect"][1]) == 11 and len(_lib.SIGNATURES["dinox_ntxent_coeff_rect"][1]) == 13
    assert "#define DINOX_ABI_VERSION 3" in header and _lib.lib.dinox_version() == 3          # additive: no new ABI version


def test_rect_entry_points_check_their_arguments_on_the_host():
    """Every refusal comes back as the error code with a message, ahead of any launch (the pointers below are host memory and are
    never dereferenced)."""
    from dinox import _lib
    buf = (C.c_float * 256)()
    p = C.addressof(buf)
    L = _lib.lib

    def rows(Ml=4, Mg=8, row0=4, Bl=2, inv_tau=10.0, lds=8, S=p, out=p):
        return L.dinox_ntxent_rows_rect(S, lds, Ml, Mg, row0, Bl, inv_tau, out, out, out, None)

    def coeff(Ml=4, Mg=8, row0=4, Bl=2, inv_tau=10.0, lds=8, ldw=8, lse_all=p, W=p + 512):
        return L.dinox_ntxent_coeff_rect(p, lds, p, lse_all, Ml, Mg, row0, Bl, inv_tau, 1.0, W, ldw, None)

    for fn in (rows, coeff):
        for bad, word in ((dict(Ml=5, Bl=2), "Ml=5"), (dict(Ml=0, Bl=0), "Ml=0"), (dict(Ml=1, Bl=0), "Ml=1"), (dict(Mg=10), "Mg=10"),
                          (dict(Mg=0), "Mg=0"), (dict(row0=2), "row0=2"), (dict(row0=8), "row0=8"), (dict(row0=-4), "row0=-4"),
                          (dict(Bl=1), "Bl=1"), (dict(Bl=4), "Bl=4"), (dict(inv_tau=0.0), "inv_tau"), (dict(inv_tau=-1.0), "inv_tau"),
                          (dict(inv_tau=float("nan")), "inv_tau"), (dict(lds=7), "lds=7")):
            assert fn(**bad) == -1 and word in _lib.last_error(), (fn.__name__, bad, _lib.last_error())
    assert rows(S=None) == -1 and "null" in _lib.last_error()
    assert rows(out=None) == -1 and "null" in _lib.last_error()
    assert coeff(lse_all=None) == -1 and "null" in _lib.last_error()
    assert coeff(W=None) == -1 and "null" in _lib.last_error()
    assert coeff(ldw=7) == -1 and "ldw=7" in _lib.last_error()


def test_ops_keep_their_refusals_with_the_new_arguments():
    import torch
    from dinox import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ntxent_fwd(torch.randn(4, 8), 0.1, group=None, force_rect=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.simclr_loss(torch.randn(2, 8), torch.randn(2, 8), 0.1, group=None, force_rect=True)
