"""GPU tests of the boundary loss: csrc/distmap.hip against the brute-force float64 oracle (tests/_bdloss_oracle.py) within the derived
3 * 2^-24 relative bound at every element, its zero planes, ignore handling, sign and bit equalities; the boundary term of
csrc/segloss.hip against the float64 oracle within a-priori bounds, its exact properties (phi times two, w_bd = 0 against the old entry
points, all ignored, run to run), ops.SegBoundaryLossFn under autograd, and scripts/finetune_segmentation.py with the boundary flags.

Distance-map shapes: [2, 37, 70] crosses a wave, [1, 5, 300] the 256-thread block along x, [1, 3, 256] / [1, 3, 257] sit on either side
of the one-wave / four-wave row kernels, [1, 1024, 3] and [1, 3, 1024] reach the side limit and the uint16 range, [1, 1, 1] is the
smallest map."""
import importlib.util
import json
import os
import sys

import numpy as np
import pytest
import torch

import _bdloss_oracle as BO
import _segloss_oracle as SO
from conftest import ROOT

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RATIOS: dict = {}


# ------------------------------------------------------------------------------------------ label maps
def make_map(kind, rng, B, H, W, C):
    if kind == "blobs":                                      # C - 1 ellipses over class 0, later ones on top
        y = np.zeros((B, H, W), dtype=np.uint8)
        yy, xx = np.mgrid[0:H, 0:W]
        for b in range(B):
            for c in range(1, C):
                cy, cx = rng.uniform(0, H), rng.uniform(0, W)
                ry, rx = rng.uniform(0.15, 0.4) * max(H, 2), rng.uniform(0.15, 0.4) * max(W, 2)
                y[b][((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = c
        return y
    if kind == "single pixel":                               # class C - 1 is one pixel per image, the rest random among the others
        y = rng.integers(0, C - 1, (B, H, W)).astype(np.uint8)
        for b in range(B):
            y[b, rng.integers(0, H), rng.integers(0, W)] = C - 1
        return y
    if kind == "checkerboard":
        yy, xx = np.mgrid[0:H, 0:W]
        return np.broadcast_to(((yy + xx) % C).astype(np.uint8), (B, H, W)).copy()
    raise AssertionError(kind)


def device_phi(y, spacing, C):
    from dinox import ops
    return ops.signed_distance_map(torch.from_numpy(y).to(DEV), torch.tensor(spacing, dtype=torch.float32), C)


def judge_phi(name, got, ref):
    """Every element: |got - exact| <= 3 u exact (so an exact 0 must be 0), the sign included."""
    got = got.double().cpu().numpy()
    assert got.shape == ref.shape and np.isfinite(got).all()
    err, bound = np.abs(got - ref), BO.DIST_REL * np.abs(ref)
    nz = bound > 0
    ratio = float((err[nz] / bound[nz]).max()) if nz.any() else 0.0
    print(f"{name}: largest error / bound = {ratio:.4g} over {int(nz.sum())} non-zero distances")
    RATIOS["phi"] = max(RATIOS.get("phi", 0.0), ratio)
    assert (err <= bound).all(), f"{name}: error / bound = {ratio:.3g}; {int((err > bound).sum())} element(s) outside, first at {np.argwhere(err > bound)[0]}"


SHAPES = ((2, 37, 70), (1, 5, 300), (1, 3, 256), (1, 3, 257), (1, 1024, 3), (1, 3, 1024), (1, 1, 1))


@pytest.mark.parametrize("kind", ["blobs", "single pixel", "checkerboard"])
@pytest.mark.parametrize("C", [2, 3, 5])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_distance_map_against_brute_force(shape, C, kind):
    B, H, W = shape
    rng = np.random.default_rng([B, H, W, C, len(kind)])
    y = make_map(kind, rng, B, H, W, C)
    spacing = rng.uniform(0.4, 2.5, (B, 2)).astype(np.float32)
    judge_phi(f"{kind} {shape} C={C}", device_phi(y, spacing, C), BO.signed_distance(y, spacing, C))


def test_anisotropy_and_per_image_spacing():
    """The query is pixel (0, 0); one class-1 pixel four rows down its column, another two columns along its row.  With spacing (1, 1)
    the nearest is the one along the row (2 against 4); with (0.5, 2.5) it is the one BELOW (2.0 against 5.0), which the isotropic
    transform would not pick; with (2.5, 0.5) the one along the row again (1.0 against 10.0).  The three images of one batch differ
    only in their spacing."""
    y = np.zeros((3, 6, 9), dtype=np.uint8)
    y[:, 4, 0] = 1
    y[:, 0, 2] = 1
    spacing = np.array([[0.5, 2.5], [1.0, 1.0], [2.5, 0.5]], dtype=np.float32)
    got = device_phi(y, spacing, 2)
    ref = BO.signed_distance(y, spacing, 2)
    assert ref[:, 1, 0, 0].tolist() == [2.0, 2.0, 1.0] and ref[0, 1, 0, 1] == 2.5 and ref[1, 1, 0, 1] == 1.0
    judge_phi("anisotropy", got, ref)
    assert got[:, 1, 0, 0].tolist() == [2.0, 2.0, 1.0]


def test_zero_planes_and_ignore():
    y = np.zeros((2, 9, 11), dtype=np.uint8)
    y[0, 3:6, 2:7] = 2                                       # image 0: class 1 absent; image 1: class 0 covers every valid pixel
    y[1, :, 5] = 255
    y[0, 0, :] = 255
    got = device_phi(y, np.array([[1.5, 0.7], [1.0, 1.0]], dtype=np.float32), 3).cpu().numpy()
    assert not got[0, 1].view(np.uint32).any(), "an absent class has an exactly zero plane"
    assert not got[1].view(np.uint32).any(), "a class that covers every valid pixel, and the absent ones, have exactly zero planes"
    assert not got[0, :, 0, :].view(np.uint32).any(), "ignored pixels are 0 in every plane"
    judge_phi("zero planes", torch.from_numpy(got), BO.signed_distance(y, np.array([[1.5, 0.7], [1.0, 1.0]], dtype=np.float32), 3))
    # ignored pixels are no sources: the query's neighbours of the other kind are ignored, the distance reaches past them
    y = np.zeros((1, 1, 8), dtype=np.uint8)
    y[0, 0, 1:4] = 255
    y[0, 0, 4:] = 1
    got = device_phi(y, np.array([[1.0, 1.0]], dtype=np.float32), 2).cpu().numpy()
    assert got[0, 1, 0].tolist() == [4.0, 0.0, 0.0, 0.0, -4.0, -5.0, -6.0, -7.0]
    assert got[0, 0, 0].tolist() == [-4.0, 0.0, 0.0, 0.0, 4.0, 5.0, 6.0, 7.0]


def test_sign_and_smallest_distance():
    rng = np.random.default_rng(11)
    y = make_map("blobs", rng, 2, 40, 52, 3)
    y[:, 0, 0], y[:, 1, 1], y[:, 2, 2] = 0, 1, 2            # every class present in both images
    y[rng.random(y.shape) < 0.05] = 255
    spacing = np.array([[0.6, 1.7], [2.0, 0.9]], dtype=np.float32)
    got = device_phi(y, spacing, 3).cpu().numpy()
    for c in range(3):
        inside, outside = y == c, (y != c) & (y != 255)
        assert (got[:, c][inside] < 0).all() and (got[:, c][outside] > 0).all() and (got[:, c][y == 255] == 0).all()
        for b in range(2):
            valid = y[b] != 255
            assert (np.abs(got[b, c][valid]) >= spacing[b].min()).all()


def test_distance_map_bit_equalities():
    rng = np.random.default_rng(5)
    y = make_map("blobs", rng, 3, 33, 47, 2)
    y[rng.random(y.shape) < 0.1] = 255
    spacing = rng.uniform(0.4, 2.5, (3, 2)).astype(np.float32)
    a, b = device_phi(y, spacing, 2), device_phi(y, spacing, 2)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "run to run"
    alone = device_phi(y[1:2], spacing[1:2], 2)
    assert torch.equal(alone.view(torch.int32), a[1:2].view(torch.int32)), "an image alone against the same image inside a batch"
    five = device_phi(y, spacing, 5)                        # labels 0, 1 and 255 only: the sets of classes 0 and 1 are those of C = 2
    assert torch.equal(five[:, :2].view(torch.int32), a.view(torch.int32)), "a class under C = 5 against the same sets under C = 2"
    assert not five[:, 2:].view(torch.int32).any()


def test_bad_label_is_refused():
    from dinox import ops
    y = torch.zeros((1, 6, 6), dtype=torch.uint8, device=DEV)
    y[0, 2, 3] = 7
    with pytest.raises(ValueError, match="1 label"):
        ops.signed_distance_map(y, [[1.0, 1.0]], 3)
    with pytest.raises(ValueError, match="num_classes"):
        ops.signed_distance_map(y, [[1.0, 1.0]], 65)
    with pytest.raises(ValueError, match="spacing"):
        ops.signed_distance_map(y, [[1.0, 0.0]], 3)


def test_scipy_is_a_second_witness_at_224():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(224)
    y = make_map("blobs", rng, 2, 224, 224, 3)
    y[:, 0, 0], y[:, 1, 1], y[:, 2, 2] = 0, 1, 2
    spacing = np.array([[0.8, 1.3], [1.0, 1.0]], dtype=np.float32)
    judge_phi("scipy 224 x 224", device_phi(y, spacing, 3), BO.scipy_signed_distance(y, spacing, 3, ndi))


# ------------------------------------------------------------------------------------------ the loss
LOSS_SHAPES = ((3, 4, 3), (5, 7, 2), (4, 8, 5), (2, 32, 3), (2, 2, 64))          # (g, u, C)
TRIPLES = ((1.0, 1.0, 0.5), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0))
_CASES: dict = {}


def loss_case(g, u, C):
    """(z, y, phi on the device, their host copies), made once per shape and left unchanged: B = 2, some columns ignored, phi from
    ops.signed_distance_map with a non-unit spacing."""
    if (g, u, C) not in _CASES:
        rng = np.random.default_rng([g, u, C])
        B, S = 2, g * u
        z = (rng.standard_normal((B, g * g, C)) * 3).astype(np.float32)
        y = rng.integers(0, C, (B, S, S)).astype(np.uint8)
        if S >= 8:                                           # coarse structure, so the distances are not all about one pixel
            y[:, : S // 2, : S // 3] = 0
            y[:, S // 2:, S // 2:] = C - 1
        y[:, :, 1] = 255
        y[0, :, S - 1] = 255
        zt, yt = torch.from_numpy(z).to(DEV), torch.from_numpy(y).to(DEV)
        phi = device_phi(y, np.array([[0.7, 1.9], [1.3, 0.6]], dtype=np.float32), C)
        _CASES[(g, u, C)] = (zt, yt, phi, z, y, phi.cpu().numpy(), SO.Pixels(z, y, g, u))
    return _CASES[(g, u, C)]


def judge(name, got, ref, bound):
    got = got.detach().double().cpu().numpy().reshape(ref.shape)
    assert np.isfinite(got).all(), f"{name}: non-finite output"
    err = np.abs(got - ref)
    ratio = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print(f"{name}: error / bound = {ratio:.4g}")
    RATIOS[name] = max(RATIOS.get(name, 0.0), ratio)
    assert (err <= bound).all(), f"{name}: error / bound = {ratio:.3g} at {np.unravel_index((err / np.maximum(bound, 1e-300)).argmax(), err.shape)}"


@pytest.mark.parametrize("c0", [0, 1])
@pytest.mark.parametrize("g,u,C", LOSS_SHAPES)
def test_loss_against_the_oracle(g, u, C, c0):
    from dinox import ops
    zt, yt, phi, z, y, ph, px = loss_case(g, u, C)
    for w_ce, w_dice, w_bd in TRIPLES:
        loss, stats, saved = ops.seg_loss_bd_fwd(zt, yt, phi, w_ce, w_dice, w_bd, c0)
        dz = ops.seg_loss_bd_bwd(saved, 1.0)
        fwd = BO.forward(z, y, ph, g, u, w_ce, w_dice, w_bd, c0, px)
        ref_dz, e_dz = BO.backward(z, y, ph, g, u, w_ce, w_dice, w_bd, c0, 1.0, px, fwd)
        assert saved[4].tolist() == [fwd["nv"], 0]
        for i, what in enumerate(("L", "CE", "Dice", "BD")):
            judge(f"fwd {what}", loss[i], fwd["loss"][i:i + 1], fwd["e_loss"][i:i + 1])
        judge("fwd stats", stats, fwd["stats"], fwd["e_stats"])
        judge("bwd dz", dz, ref_dz, e_dz)


@pytest.mark.parametrize("g,u,C", [(3, 4, 3), (4, 8, 5), (2, 2, 64)])
def test_twice_phi_doubles_the_boundary_term_exactly(g, u, C):
    from dinox import ops
    zt, yt, phi, *_ = loss_case(g, u, C)
    l1, _, s1 = ops.seg_loss_bd_fwd(zt, yt, phi, 0.0, 0.0, 1.0, 1)
    l2, _, s2 = ops.seg_loss_bd_fwd(zt, yt, phi * 2, 0.0, 0.0, 1.0, 1)
    assert torch.equal(l2[[0, 3]], 2 * l1[[0, 3]]) and float(l1[3]) != 0.0 and torch.equal(l1[0], l1[3])
    d1, d2 = ops.seg_loss_bd_bwd(s1), ops.seg_loss_bd_bwd(s2)
    assert torch.equal(d2, 2 * d1) and bool(d1.abs().max() > 0)


@pytest.mark.parametrize("c0", [0, 1])
@pytest.mark.parametrize("g,u,C", LOSS_SHAPES)
def test_zero_weight_keeps_the_bits_of_the_old_entry_points(g, u, C, c0):
    from dinox import ops
    zt, yt, phi, z, y, ph, px = loss_case(g, u, C)
    old, old_stats, old_saved = ops.seg_loss_fwd(zt, yt, 0.7, 1.3, c0)
    new, new_stats, new_saved = ops.seg_loss_bd_fwd(zt, yt, phi, 0.7, 1.3, 0.0, c0)
    assert torch.equal(new[:3].view(torch.int32), old.view(torch.int32)) and torch.equal(new_stats.view(torch.int32), old_stats.view(torch.int32))
    assert torch.equal(ops.seg_loss_bd_bwd(new_saved, -2.5).view(torch.int32), ops.seg_loss_bwd(old_saved, -2.5).view(torch.int32))
    fwd = BO.forward(z, y, ph, g, u, 0.7, 1.3, 0.0, c0, px)  # BD is reported all the same
    judge("fwd BD", new[3], fwd["loss"][3:], fwd["e_loss"][3:])
    assert float(new[3]) != 0.0


def test_all_ignored_is_exactly_zero():
    from dinox import ops
    zt, yt, phi, *_ = loss_case(3, 4, 3)
    loss, _, saved = ops.seg_loss_bd_fwd(zt, torch.full_like(yt, 255), phi, 1.0, 1.0, 0.5, 0)
    assert not loss.view(torch.int32).any() and not ops.seg_loss_bd_bwd(saved).view(torch.int32).any()


@pytest.mark.parametrize("g,u,C", [(4, 8, 5), (2, 32, 3)])
def test_two_calls_give_the_same_bits(g, u, C):
    from dinox import ops
    zt, yt, phi, *_ = loss_case(g, u, C)
    outs = []
    for _ in range(2):
        loss, stats, saved = ops.seg_loss_bd_fwd(zt, yt, phi, 1.0, 1.0, 0.5, 1)
        outs.append((loss.clone(), stats.clone(), ops.seg_loss_bd_bwd(saved)))
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(*outs))


def test_autograd_node():
    from dinox import ops
    zt, yt, phi, *_ = loss_case(4, 8, 5)
    z = zt.clone().requires_grad_(True)
    ph = phi.clone().requires_grad_(True)
    L, ce, dice, bd = ops.SegBoundaryLossFn.apply(z, yt, ph, 1.0, 1.0, 0.5, 1)
    assert L.requires_grad and not (ce.requires_grad or dice.requires_grad or bd.requires_grad)
    (3.0 * L).backward()
    _, _, saved = ops.seg_loss_bd_fwd(zt, yt, phi, 1.0, 1.0, 0.5, 1)
    assert torch.equal(z.grad, ops.seg_loss_bd_bwd(saved, 1.0) * 3.0) and ph.grad is None
    got = ops.SegBoundaryLossFn.backward(type("Ctx", (), {"saved": saved, "zdt": torch.float32})(), torch.tensor(1.0, device=DEV))
    assert len(got) == 7 and all(v is None for v in got[1:])      # y, phi and the four numbers receive None
    zb = zt.bfloat16().requires_grad_(True)
    ops.SegBoundaryLossFn.apply(zb, yt, phi, 1.0, 1.0, 0.5, 0)[0].backward()
    assert zb.grad.dtype == torch.bfloat16 and bool(zb.grad.float().abs().max() > 0)
    with pytest.raises(ValueError, match="phi must be fp32"):
        ops.seg_loss_bd_fwd(zt, yt, phi[:, :2])


# ------------------------------------------------------------------------------------------ scripts/finetune_segmentation.py
TINY = dict(img_size=32, patch=8, dim=32, depth=2, heads=2, scale_aware=True)      # the configuration tests/test_segloss_gpu.py trains


def _script():
    if "finetune_segmentation" in sys.modules:
        return sys.modules["finetune_segmentation"]
    spec = importlib.util.spec_from_file_location("finetune_segmentation", os.path.join(ROOT, "dino-x_amd", "scripts", "finetune_segmentation.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def backbone_dir(tmp_path_factory):
    import zoo.arch as arch
    from zoo.hub import export_hub_checkpoint
    torch.manual_seed(0)
    m = arch.PatchViT(**TINY)
    with torch.no_grad():
        m.scale_embed.mlp[2].weight.normal_(0, 0.05)
    d = tmp_path_factory.mktemp("tiny_hub_bd")
    export_hub_checkpoint(m.to(DEV).eval(), d, config=dict(TINY, mlp_ratio=4.0, num_registers=4))
    return d


def _run(backbone_dir, out, *extra, through_cli=True):
    fs = _script()
    argv = ["--backbone", str(backbone_dir), "--synthetic", "48", "--num-classes", "3", "--epochs", "3", "--batch-size", "12", "--rank", "0",
            "--lr", "1e-2", "--warmup-epochs", "1", "--seed", "0", "--output", str(out), *extra]
    return fs.run(fs.parse_cli(argv) if through_cli else fs.build_parser().parse_args(argv))


@pytest.mark.parametrize("units", ["px", "mm"])
def test_script_trains_with_the_boundary_term(backbone_dir, tmp_path, units):
    res = _run(backbone_dir, tmp_path, "--boundary-weight", "0.5", "--boundary-ramp-epochs", "2", "--boundary-units", units)
    cfg = res["config"]
    print(f"{units}: train loss per epoch {cfg.train_loss_history}, best validation metrics {cfg.best_val_metrics}")
    assert len(cfg.train_loss_history) == 3 and np.isfinite(cfg.train_loss_history).all() and np.isfinite(cfg.best_val_loss)
    saved = json.loads((tmp_path / "finetune_config.json").read_text())
    assert (saved["boundary_weight"], saved["boundary_ramp_epochs"], saved["boundary_units"]) == (0.5, 2, units)


def test_script_without_the_flags_and_with_weight_zero_agree(backbone_dir, tmp_path):
    a = _run(backbone_dir, tmp_path / "a", through_cli=False)["config"]      # a namespace without the boundary attributes: off
    b = _run(backbone_dir, tmp_path / "b", "--boundary-weight", "0", "--boundary-units", "mm")["config"]
    assert a.train_loss_history == b.train_loss_history and a.best_val_metrics == b.best_val_metrics and a.best_epoch == b.best_epoch
    assert (b.boundary_weight, a.boundary_weight) == (0.0, 0.0)


def test_zz_report_error_to_bound_ratios():
    """Not a check of its own: prints the largest error / bound ratio every test above saw (each was asserted <= 1 there)."""
    for k in sorted(RATIOS):
        print(f"{k}: largest error / bound = {RATIOS[k]:.4g}")
