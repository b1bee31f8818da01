"""CPU checks of the boundary loss: the brute-force distance oracle (tests/_bdloss_oracle.py) against scipy's Euclidean transform and on
hand-made 5 x 5 maps, the float64 loss oracle against the framework statement under autograd, the host-side refusals and workspace
formula of the new entry points (no kernel is launched), and the command line of scripts/finetune_segmentation.py."""
import importlib.util
import logging
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _bdloss_oracle as BO
from conftest import ROOT


# ------------------------------------------------------------------------------------------ the distance oracle
@pytest.mark.parametrize("spacing", [(1.0, 1.0), (0.5, 2.5)])
def test_brute_force_is_the_scipy_expression(spacing):
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(1)
    y = (rng.random((2, 19, 23)) < 0.3).astype(np.uint8) + (rng.random((2, 19, 23)) < 0.1).astype(np.uint8)
    sp = np.array([spacing, spacing[::-1]], dtype=np.float32)
    got, want = BO.signed_distance(y, sp, 3), BO.scipy_signed_distance(y, sp, 3, ndi)
    assert np.abs(got).max() > 1 and np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_oracle_on_hand_made_maps():
    y = np.zeros((1, 5, 5), dtype=np.uint8)
    y[0, 2, 2] = 1
    phi = BO.signed_distance(y, [[1.0, 1.0]], 3)
    assert phi[0, 1, 2, 2] == -1.0 and phi[0, 1, 0, 0] == np.sqrt(8.0) and phi[0, 1, 2, 0] == 2.0       # inside: to the nearest outside pixel
    assert phi[0, 0, 2, 2] == 1.0 and phi[0, 0, 0, 0] == -np.sqrt(8.0) and phi[0, 0, 2, 1] == -1.0
    assert not phi[0, 2].any()                               # class 2 is absent: the empty-set rule
    y[:] = 1
    assert not BO.signed_distance(y, [[1.0, 1.0]], 3).any()  # class 1 covers everything: no pixel has a set to measure to
    # ignore: neither a source nor a query; the pixel next to the centre is ignored, the distance reaches past it
    y = np.zeros((1, 5, 5), dtype=np.uint8)
    y[0, 2, 2] = 1
    y[0, 2, 1] = y[0, 2, 3] = y[0, 1, 2] = y[0, 3, 2] = 255
    phi = BO.signed_distance(y, [[1.0, 1.0]], 2)
    assert phi[0, 1, 2, 2] == -np.sqrt(2.0) and phi[0, 1, 2, 1] == 0.0 and phi[0, 0, 2, 1] == 0.0 and phi[0, 0, 1, 1] == -np.sqrt(2.0)
    y[:] = 255
    y[0, 0, 0] = 0                                           # one valid pixel: class 0 covers every valid pixel
    assert not BO.signed_distance(y, [[1.0, 1.0]], 2).any()
    # the image edge is no boundary: a class cut by the crop measures to the other pixels only
    y = np.zeros((1, 5, 5), dtype=np.uint8)
    y[0, :, :2] = 1
    assert BO.signed_distance(y, [[3.0, 0.5]], 2)[0, 1, 0].tolist() == [-1.0, -0.5, 0.5, 1.0, 1.5]
    with pytest.raises(AssertionError):
        BO.signed_distance(np.full((1, 2, 2), 7, dtype=np.uint8), [[1.0, 1.0]], 3)


# ------------------------------------------------------------------------------------------ the loss oracle
def torch_statement(z, y, phi, g, u, w_ce, w_dice, w_bd, c0):
    z = torch.from_numpy(z).double().requires_grad_(True)
    yt = torch.from_numpy(y.astype(np.int64))
    B, P, C = z.shape
    logits = F.interpolate(z.reshape(B, g, g, C).permute(0, 3, 1, 2), scale_factor=u, mode="bilinear", align_corners=False)
    valid = yt != 255
    ce = F.cross_entropy(logits, yt, ignore_index=255)
    p = logits.softmax(1) * valid[:, None]
    oh = torch.stack([(yt == c) & valid for c in range(C)], 1).double()
    I, Pc, Y = (p * oh).sum((0, 2, 3)), p.sum((0, 2, 3)), oh.sum((0, 2, 3))
    dice = 1 - ((2 * I + 1) / (Pc + Y + 1))[c0:].mean()
    bd = (p * torch.from_numpy(phi))[:, c0:].sum() / (valid.sum() * (C - c0))   # the mean of p phi over the valid pixels and the classes >= c0
    L = w_ce * ce + w_dice * dice + w_bd * bd
    L.backward()
    return torch.stack([L, ce, dice, bd]).detach().numpy(), z.grad.numpy()


@pytest.mark.parametrize("g,u,C,c0,w", [(3, 4, 3, 0, (1.0, 1.0, 0.5)), (5, 7, 2, 1, (0.0, 0.0, 1.0)), (2, 8, 5, 1, (0.7, 1.3, 2.0)), (2, 2, 64, 0, (1.0, 0.0, 0.0))])
def test_loss_oracle_is_the_framework_statement(g, u, C, c0, w):
    rng = np.random.default_rng([g, u, C])
    B, S = 2, g * u
    z = rng.standard_normal((B, g * g, C)) * 3
    y = rng.integers(0, C, (B, S, S)).astype(np.uint8)
    y[:, :, 1] = 255
    phi = BO.signed_distance(y, [[0.7, 1.9], [1.3, 0.6]], C)
    want_loss, want_dz = torch_statement(z, y, phi, g, u, *w, c0)
    fwd = BO.forward(z, y, phi, g, u, *w, c0)
    dz, e_dz = BO.backward(z, y, phi, g, u, *w, c0)
    assert np.abs(fwd["loss"] - want_loss).max() <= 1e-10 * max(np.abs(want_loss).max(), 1e-300)
    assert np.abs(dz - want_dz).max() <= 1e-10 * max(np.abs(want_dz).max(), 1e-300)
    assert (fwd["e_loss"] >= 0).all() and (fwd["e_loss"] < 1e-3).all() and (e_dz >= 0).all() and e_dz.max() < 1e-3 * max(np.abs(dz).max(), 1.0)
    two = BO.backward(z, y, phi, g, u, *w, c0, grad_scale=-2.5)[0]
    assert np.abs(two + 2.5 * want_dz).max() <= 1e-10 * max(np.abs(want_dz).max(), 1e-300)


def test_loss_oracle_edge_cases():
    rng = np.random.default_rng(9)
    z = rng.standard_normal((1, 4, 3))
    y = rng.integers(0, 3, (1, 8, 8)).astype(np.uint8)
    phi = BO.signed_distance(y, [[1.0, 1.0]], 3)
    none = np.full_like(y, 255)
    assert not BO.forward(z, none, phi, 2, 4)["loss"].any() and not BO.backward(z, none, phi, 2, 4)[0].any()
    # c0 = 1: plane 0 is not read
    other = phi.copy()
    other[:, 0] = 1e6
    assert np.array_equal(BO.forward(z, y, phi, 2, 4, c0=1)["loss"], BO.forward(z, y, other, 2, 4, c0=1)["loss"])
    assert np.array_equal(BO.backward(z, y, phi, 2, 4, c0=1)[0], BO.backward(z, y, other, 2, 4, c0=1)[0])
    # a perfect, confident prediction sits inside its regions: BD is negative
    zz = np.zeros((1, 4, 2))
    yy = np.zeros((1, 4, 4), dtype=np.uint8)
    yy[0, :, 2:] = 1
    zz[0, [0, 2], 0] = zz[0, [1, 3], 1] = 30.0
    assert BO.forward(zz, yy, BO.signed_distance(yy, [[1.0, 1.0]], 2), 2, 2)["loss"][3] < -0.5


# ------------------------------------------------------------------------------------------ entry points: host-side checks, no launch
def test_signed_distance_refusals_and_workspace():
    from dinox import _lib
    lib, p = _lib.lib, 4096                                  # a non-null pointer value: refusals come before anything is dereferenced

    def call(H, W, C, y=p, sp=p, phi=p, bad=p, ws=p, B=1):
        return lib.dinox_signed_distance(y, sp, phi, bad, ws, B, H, W, C, None)

    for H, W in ((0, 8), (8, 0), (1025, 8), (8, 1025)):
        assert call(H, W, 3) == -1 and "1 <= H, W <= 1024" in _lib.last_error()
        assert lib.dinox_signed_distance_ws_bytes(1, H, W, 3) == 0
    assert call(8, 8, 1) == -1 and "C=1" in _lib.last_error()
    assert call(8, 8, 65) == _lib.EUNSUPPORTED and "C=65" in _lib.last_error()
    assert call(8, 8, 3, B=0) == -1 and "B=0" in _lib.last_error()
    for null in ("y", "sp", "phi", "bad", "ws"):
        assert call(8, 8, 3, **{null: None}) == -1 and "null pointer" in _lib.last_error()
    for B, H, W, C in ((1, 1, 1, 2), (2, 37, 70, 3), (8, 1024, 1024, 3), (5, 224, 224, 64)):
        assert lib.dinox_signed_distance_ws_bytes(B, H, W, C) == 4 * B * C * H * W      # two uint16 planes per (image, class)
    assert lib.dinox_signed_distance_ws_bytes(1, 8, 8, 1) == 0 and lib.dinox_signed_distance_ws_bytes(1, 8, 8, 65) == 0
    assert lib.dinox_signed_distance_ws_bytes(0, 8, 8, 3) == 0 and lib.dinox_signed_distance_ws_bytes(1 << 20, 1024, 8, 3) == 0


def test_seg_loss_bd_refusals_and_workspace():
    from dinox import _lib
    lib, p = _lib.lib, 4096

    def fwd(g=3, u=4, C=3, c0=0, z=p, phi=p):
        return lib.dinox_seg_loss_bd_fwd(z, p, phi, p, p, p, p, 2, g, u, C, c0, 1.0, 1.0, 0.5, None)

    def bwd(g=3, u=4, C=3, c0=0, phi=p, dz=p):
        return lib.dinox_seg_loss_bd_bwd(p, p, phi, p, p, dz, p, 2, g, u, C, c0, 1.0, 1.0, 0.5, 1.0, None)

    for f in (fwd, bwd):
        assert f(phi=None) == -1 and "null pointer" in _lib.last_error()
        assert f(u=33) == -1 and "u=33" in _lib.last_error()
        assert f(C=1) == -1 and f(C=65) == _lib.EUNSUPPORTED
        assert f(c0=2) == -1 and "c0=2" in _lib.last_error()
    assert fwd(z=None) == -1 and bwd(dz=None) == -1
    for B, g, u, C in ((2, 3, 4, 3), (32, 14, 16, 3), (1, 2, 2, 64)):
        parts = -(-B * g * g // 8)
        want = max(parts * (2 + 2 * C) * 4 + parts * (C + 2) * 4, B * g * g * 4 * C * 4)
        assert lib.dinox_seg_loss_bd_ws_bytes(B, g, u, C) == want >= lib.dinox_seg_loss_ws_bytes(B, g, u, C)
    assert lib.dinox_seg_loss_bd_ws_bytes(2, 3, 33, 3) == 0 and lib.dinox_seg_loss_bd_ws_bytes(2, 3, 4, 65) == 0


def test_ops_refuse_before_the_device():
    from dinox import ops
    y = torch.zeros((2, 8, 8), dtype=torch.uint8)
    with pytest.raises(ValueError, match="uint8"):
        ops.signed_distance_map(y.float(), [[1.0, 1.0]] * 2, 3)
    with pytest.raises(ValueError, match="1 <= H, W <= 1024"):
        ops.signed_distance_map(torch.zeros((1, 2, 1025), dtype=torch.uint8), [[1.0, 1.0]], 3)
    with pytest.raises(ValueError, match="num_classes"):
        ops.signed_distance_map(y, [[1.0, 1.0]] * 2, 1)
    assert ops.SegBoundaryLossFn.forward.__defaults__ == (1.0, 1.0, 1.0, 0)


# ------------------------------------------------------------------------------------------ scripts/finetune_segmentation.py
def _script():
    if "finetune_segmentation" in sys.modules:
        return sys.modules["finetune_segmentation"]
    spec = importlib.util.spec_from_file_location("finetune_segmentation", os.path.join(ROOT, "dino-x_amd", "scripts", "finetune_segmentation.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def test_boundary_flags_have_a_parser_of_their_own():
    fs = _script()
    base = {a.dest for a in fs.build_parser()._actions}
    assert not {"boundary_weight", "boundary_ramp_epochs", "boundary_units"} & base
    assert len(base) == 31                                   # help + the 30 flags tests/test_segloss_cpu.py pins by name
    a = fs.parse_cli(["--backbone", "b", "--output", "o"])
    assert (a.boundary_weight, a.boundary_ramp_epochs, a.boundary_units) == (0.0, 0, "px") and a.ce_weight == 1.0 and a.es_metric == "loss"
    a = fs.parse_cli(["--boundary-weight", "0.5", "--backbone", "b", "--boundary-units", "mm", "--output", "o", "--boundary-ramp-epochs", "3",
                      "--dice-weight", "2"])
    assert (a.boundary_weight, a.boundary_ramp_epochs, a.boundary_units, a.dice_weight, str(a.backbone)) == (0.5, 3, "mm", 2.0, "b")
    with pytest.raises(SystemExit):
        fs.parse_cli(["--backbone", "b", "--output", "o", "--boundary-units", "cm"])
    with pytest.raises(SystemExit):
        fs.build_parser().parse_args(["--backbone", "b", "--output", "o", "--boundary-weight", "1"])
    import dataclasses
    defaults = {f.name: f.default for f in dataclasses.fields(fs.SegConfig)}
    assert (defaults["boundary_weight"], defaults["boundary_ramp_epochs"], defaults["boundary_units"]) == (0.0, 0, "px")
    assert [fs.boundary_weight(0.8, 4, e) for e in range(6)] == [0.2, 0.4, pytest.approx(0.6), 0.8, 0.8, 0.8]
    assert fs.boundary_weight(0.8, 0, 0) == 0.8


@pytest.mark.parametrize("extra,what", [(["--boundary-weight", "-0.5"], "--boundary-weight"), (["--boundary-weight", "nan"], "--boundary-weight"),
                                        (["--boundary-weight", "1", "--boundary-ramp-epochs", "-1"], "--boundary-ramp-epochs")])
def test_boundary_refusals(extra, what, capsys):
    fs = _script()
    args = fs.parse_cli(["--backbone", "nowhere", "--output", "o", "--synthetic", "8", *extra])
    with pytest.raises(SystemExit):
        fs.run(args)                                        # refused before the backbone is looked for
    assert what in capsys.readouterr().err


def test_mm_without_spacing_columns_warns_and_assumes_1_mm(tmp_path, caplog):
    fs = _script()
    csv = tmp_path / "t.csv"
    csv.write_text("image_path,mask_path\na.png,a_mask.png\n")
    rows = fs.read_csv(csv)
    with caplog.at_level(logging.WARNING, logger="finetune_segmentation"):
        assert fs.warn_mm_without_spacing(rows, "mm") and "1 mm" in caplog.text
        caplog.clear()
        assert not fs.warn_mm_without_spacing(rows, "px") and not caplog.text
    assert rows[0].spacing == (1.0, 1.0, 1.0)
    csv.write_text("image_path,mask_path,spacing_x,spacing_y,spacing_z\na.png,a_mask.png,0.5,0.7,2\n")
    assert not fs.warn_mm_without_spacing(fs.read_csv(csv), "mm")


def test_grid_spacing_follows_the_transform():
    """paired_transform_grid makes paired_transform's draws and returns its pair; the factors are source pixels per output pixel."""
    fs = _script()
    g = torch.Generator().manual_seed(3)
    x, m = torch.rand((3, 40, 60), generator=g), (torch.rand((40, 60), generator=g) * 3).to(torch.uint8)
    for augment in (False, True):
        for seed in range(4):
            a = fs.paired_transform(x, m, 16, torch.Generator().manual_seed(seed), augment)
            b = fs.paired_transform_grid(x, m, 16, torch.Generator().manual_seed(seed), augment)
            assert len(a) == 2 and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
            fy, fx = b[2]
            if augment:
                assert 0 < fy <= 40 / 16 and 0 < fx <= 60 / 16
            else:
                assert (fy, fx) == (40 / 16, 60 / 24)         # the shorter side goes to 16, the longer to 24 before the crop
    ds = fs.GridSyntheticMasks(4, 16, 3, seed=0, augment=True)
    xs, sp, ms, grid = ds[1]
    assert ms.shape == (16, 16) and grid.tolist() == [sp[1].item(), sp[0].item()]
    assert len(fs.SyntheticMasks(4, 16, 3, seed=0)[1]) == 3
