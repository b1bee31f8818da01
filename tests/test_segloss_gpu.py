"""GPU tests of the dense segmentation path: csrc/segloss.hip against the float64 oracle (tests/_segloss_oracle.py) within its a-priori
bounds, determinism, ops.seg_predict, ops.SegLossFn through dinox.segment.SegHead, the memory condition, and
scripts/finetune_segmentation.py end to end.

Shapes: (g, u) = (1, 4) every tap clamped, (2, 3) an odd factor, (3, 16) an interior patch and all four borders, (14, 16) the real geometry;
C = 2, 5, 33, 64 cover the register widths 4, 8, 64 and a class count that fills none of them; z both 256-byte aligned and one float off.
The widths 16 and 32, the class counts that fill a width exactly (C = 4, 8, 16, 32), the factors 1, 2, 8, 24, 32 and the byte label and
prediction paths at u % 8 == 0 are in tests/test_seg_paths_gpu.py (case table: tests/_seg_paths_cases.py), against this module's oracle.
Every (g, u, B, C) runs label x logit regimes with c0, the loss weights and the alignment cycling through them: all fifteen regime pairs at
the three small geometries, two per (B, C) at (14, 16), which together are all fifteen."""
import importlib.util
import json
import os
import sys

import numpy as np
import pytest
import torch

import _segloss_oracle as SO
from conftest import ROOT

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GEOS = ((1, 4), (2, 3), (3, 16), (14, 16))
BS = (1, 3)
CS = (2, 5, 33, 64)
LABELS = ("random", "one class", "absent class", "quarter ignored", "all ignored")
LOGITS = ("normal", "pm80", "dominant")
WEIGHTS = ((1.0, 1.0), (0.0, 1.0), (1.0, 0.0))
REGIMES = [(lab, log) for lab in LABELS for log in LOGITS]
RATIOS: dict = {}


def make_labels(rng, regime, B, S, C):
    y = rng.integers(0, C, (B, S, S)).astype(np.uint8)
    if regime == "one class":
        y[:] = C - 1
    elif regime == "absent class":
        y[y == 1] = 0
    elif regime == "quarter ignored":
        y[rng.random((B, S, S)) < 0.25] = 255
    elif regime == "all ignored":
        y[:] = 255
    return y


def make_logits(rng, regime, B, P, C):
    if regime == "pm80":
        z = rng.choice(np.array([-80.0, 80.0], dtype=np.float32), (B, P, C))
    else:
        z = (rng.standard_normal((B, P, C)) * 3).astype(np.float32)
        if regime == "dominant":
            z[..., rng.integers(0, C)] += 40.0
    return z.astype(np.float32)


def on_device(z, offset):
    """z on the device, its storage 256-byte aligned (offset 0) or one float past that (offset 1)."""
    buf = torch.empty(z.size + 64 + offset, dtype=torch.float32, device=DEV)
    start = (-buf.data_ptr() // 4) % 64 + offset
    t = buf[start:start + z.size].view(z.shape)
    t.copy_(torch.from_numpy(z))
    assert t.data_ptr() % 256 == 4 * offset and t.is_contiguous()
    return t


def judge(name, got, ref, bound):
    got = got.detach().double().cpu().numpy().reshape(ref.shape)
    assert np.isfinite(got).all(), f"{name}: non-finite output"
    err = np.abs(got - ref)
    ratio = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print(f"{name}: error / bound = {ratio:.4g}")
    RATIOS[name] = max(RATIOS.get(name, 0.0), ratio)
    assert (err <= bound).all(), f"{name}: error / bound = {ratio:.3g} at {np.unravel_index((err / np.maximum(bound, 1e-300)).argmax(), err.shape)}"


def one_case(g, u, B, C, i, lab_regime, log_regime):
    from dinox import ops
    c0, (w_ce, w_dice), offset = i % 2, WEIGHTS[i % 3], (i // 2) % 2
    rng = np.random.default_rng([g, u, B, C, i])
    z = make_logits(rng, log_regime, B, g * g, C)
    y = make_labels(rng, lab_regime, B, g * u, C)
    zt, yt = on_device(z, offset), torch.from_numpy(y).to(DEV)
    loss, stats, saved = ops.seg_loss_fwd(zt, yt, w_ce, w_dice, c0)
    dz = ops.seg_loss_bwd(saved, 1.0)
    nv = saved[3].cpu()
    px = SO.Pixels(z, y, g, u)
    fwd = SO.forward(z, y, g, u, w_ce, w_dice, c0, px)
    ref_dz, e_dz = SO.backward(z, y, g, u, w_ce, w_dice, c0, 1.0, px, fwd)
    assert nv.tolist() == [fwd["nv"], 0]
    if lab_regime == "all ignored":                         # exactly zero, bit for bit
        assert not loss.cpu().numpy().view(np.uint32).any() and not dz.cpu().numpy().view(np.uint32).any()
        return
    assert torch.equal(stats[2].cpu().double(), torch.from_numpy(fwd["stats"][2]))      # the label counts are integers
    judge("fwd loss", loss, fwd["loss"], fwd["e_loss"])
    judge("fwd stats", stats, fwd["stats"], fwd["e_stats"])
    judge("bwd dz", dz, ref_dz, e_dz)


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("g,u", GEOS)
def test_kernels_against_the_oracle(g, u, B, C):
    if g == 14:
        k = BS.index(B) * len(CS) + CS.index(C)
        todo = [(2 * k + j) % len(REGIMES) for j in range(2)]
    else:
        todo = range(len(REGIMES))
    for i in todo:
        one_case(g, u, B, C, i, *REGIMES[i])


def test_grad_scale_and_bad_labels():
    from dinox import ops
    rng = np.random.default_rng(7)
    z, y = make_logits(rng, "normal", 2, 9, 5), make_labels(rng, "quarter ignored", 2, 48, 5)
    zt, yt = on_device(z, 0), torch.from_numpy(y).to(DEV)
    _, _, saved = ops.seg_loss_fwd(zt, yt, 0.7, 1.3, 1)
    judge("bwd dz", ops.seg_loss_bwd(saved, -2.5), *SO.backward(z, y, 3, 16, 0.7, 1.3, 1, -2.5))
    y[1, 5, 7] = 5                                          # >= C and not 255: reported, never an address
    with pytest.raises(ValueError, match="1 label"):
        ops.seg_loss_fwd(zt, torch.from_numpy(y).to(DEV))
    with pytest.raises(ValueError, match="1 label"):
        ops.seg_predict(zt, 16, torch.from_numpy(y).to(DEV))
    with pytest.raises(ValueError, match=r"C must lie in \[2, 64\]"):
        ops.seg_predict(torch.zeros(1, 4, 65, device=DEV), 4)


@pytest.mark.parametrize("g,u,B,C", [(3, 16, 3, 5), (14, 16, 3, 33), (2, 3, 1, 64)])
def test_two_calls_give_the_same_bits(g, u, B, C):
    from dinox import ops
    rng = np.random.default_rng([9, g, C])
    zt = on_device(make_logits(rng, "normal", B, g * g, C), 1)
    yt = torch.from_numpy(make_labels(rng, "quarter ignored", B, g * u, C)).to(DEV)
    outs = []
    for _ in range(2):
        loss, stats, saved = ops.seg_loss_fwd(zt, yt, 1.0, 1.0, 1)
        outs.append((loss.clone(), stats.clone(), ops.seg_loss_bwd(saved, 1.0).clone()))
        torch.empty(1 << 20, device=DEV).normal_()          # other work between the calls
    assert all(torch.equal(a, b) for a, b in zip(*outs))


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("g,u", GEOS)
def test_predict(g, u, C):
    from dinox import ops
    for B in BS:
        rng = np.random.default_rng([11, g, u, B, C])
        z = make_logits(rng, "normal", B, g * g, C)
        y = make_labels(rng, "quarter ignored", B, g * u, C)
        ref, margin, e_l = SO.predict(z, g, u)
        decided = margin > e_l
        share = 1.0 - decided.mean()
        print(f"predict g={g} u={u} B={B} C={C}: {share:.2%} of the pixels undecided in float64")
        assert share <= 0.01
        pred, counts = ops.seg_predict(on_device(z, B % 2), u, torch.from_numpy(y).to(DEV))
        pred = pred.cpu().numpy()
        assert pred.dtype == np.uint8 and pred.shape == ref.shape and (pred[decided] == ref[decided]).all()
        assert np.array_equal(counts.cpu().numpy(), SO.counts(pred, y, C))
        assert torch.equal(ops.seg_predict(on_device(z, 0), u).cpu(), torch.from_numpy(pred))      # without labels: the same map
    tie = torch.zeros((1, g * g, C), device=DEV)            # an exact tie everywhere: the lowest index
    assert not ops.seg_predict(tie, u).any()


def _torch_statement(tokens, weight, bias, y, g, u, w_ce, w_dice, c0):
    import torch.nn.functional as F
    w, b = weight.double().requires_grad_(True), bias.double().requires_grad_(True)
    z = tokens.double() @ w.t() + b
    B, P, C = z.shape
    logits = F.interpolate(z.reshape(B, g, g, C).permute(0, 3, 1, 2), scale_factor=u, mode="bilinear", align_corners=False)
    yl = y.long()
    valid = yl != 255
    ce = F.cross_entropy(logits, yl, ignore_index=255)
    p = logits.softmax(1) * valid[:, None]
    oh = torch.stack([(yl == c) & valid for c in range(C)], 1).double()
    D = (2 * (p * oh).sum((0, 2, 3)) + 1) / (p.sum((0, 2, 3)) + oh.sum((0, 2, 3)) + 1)
    L = w_ce * ce + w_dice * (1 - D[c0:].mean())
    L.backward()
    return L.detach(), w.grad, b.grad


def test_autograd_through_the_head():
    """SegLossFn through SegHead in fp32 mode against the float64 framework statement.  Tolerance: dW = dz^T tokens over B P = 48 rows
    of K = 32 columns; dz carries the kernel's bound (<= ~1e-5 relative of its scale here, printed by the oracle tests), the logits one
    fp32 GEMM (gam(32)); a relative 1e-4 of the largest gradient entry covers both with an order of magnitude to spare and is three
    orders below a wrong gradient."""
    from dinox import ops
    from dinox.segment import SegHead
    g, u, B, C, D = 4, 8, 3, 5, 32
    gen = torch.Generator().manual_seed(3)
    tokens = torch.randn(B, 1 + g * g + 4, D, generator=gen).to(DEV)
    y = torch.from_numpy(make_labels(np.random.default_rng(5), "quarter ignored", B, g * u, C)).to(DEV)
    torch.manual_seed(1)
    head = SegHead(D, C).to(DEV)
    with torch.no_grad():
        head.proj.bias.normal_(0, 0.5)
    with ops.compute_dtype(torch.float32):
        total, ce, dice = ops.SegLossFn.apply(head(tokens, g * g), y, 0.7, 1.3, 1)
        assert not ce.requires_grad and not dice.requires_grad
        (2.0 * total).backward()
    L, dw, db = _torch_statement(tokens[:, 1:1 + g * g].cpu(), head.proj.weight.detach().cpu(), head.proj.bias.detach().cpu(), y.cpu(), g, u,
                                 0.7, 1.3, 1)
    assert abs(float(total.detach()) - float(L)) <= 1e-5 * abs(float(L))
    for name, got, ref in (("weight", head.proj.weight.grad, 2 * dw), ("bias", head.proj.bias.grad, 2 * db)):
        err = (got.double().cpu() - ref).abs().max().item()
        RATIOS[f"autograd d{name}"] = err / (1e-4 * ref.abs().max().item())
        assert err <= 1e-4 * ref.abs().max().item(), (name, err)


def test_no_full_resolution_tensor_is_allocated():
    from dinox import ops
    B, C, g, u = 4, 16, 14, 16
    S = g * u
    rng = np.random.default_rng(13)
    z = on_device(make_logits(rng, "normal", B, g * g, C), 0).requires_grad_(True)
    y = torch.from_numpy(make_labels(rng, "quarter ignored", B, S, C)).to(DEV)
    for timed in (False, True):                             # once to warm the allocator and the code objects
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        total, _, _ = ops.SegLossFn.apply(z, y, 1.0, 1.0, 0)
        total.backward()
        torch.cuda.synchronize()
        extra = torch.cuda.max_memory_allocated() - before
        z.grad = None
    print(f"peak extra device memory of one forward + backward: {extra} bytes; one full-resolution fp32 channel: {B * S * S * 4}")
    assert extra < B * S * S * 4


# ------------------------------------------------------------------------------------------ scripts/finetune_segmentation.py
TINY = dict(img_size=32, patch=8, dim=32, depth=2, heads=2, scale_aware=True)      # the configuration tests/test_lora_gpu.py trains


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
    d = tmp_path_factory.mktemp("tiny_hub_seg")
    export_hub_checkpoint(m.to(DEV).eval(), d, config=dict(TINY, mlp_ratio=4.0, num_registers=4))
    return d


def _run(fs, backbone_dir, out, rank):
    argv = ["--backbone", str(backbone_dir), "--synthetic", "48", "--num-classes", "3", "--epochs", "4", "--batch-size", "12", "--rank", str(rank),
            "--lr", "1e-2", "--warmup-epochs", "1", "--seed", "0", "--output", str(out)]
    return fs.run(fs.build_parser().parse_args(argv))


@pytest.fixture(scope="module", params=[0, 4], ids=["rank0", "rank4"])
def first_run(request, backbone_dir, tmp_path_factory):
    out = tmp_path_factory.mktemp(f"seg_rank{request.param}")
    return request.param, out, _run(_script(), backbone_dir, out, request.param)


def test_script_trains_and_writes_its_files(first_run):
    rank, out, res = first_run
    hist = res["config"].train_loss_history
    print(f"rank {rank}: train loss per epoch {hist}, best validation metrics {res['config'].best_val_metrics}")
    assert len(hist) == 4 and hist[-1] < hist[0]
    want = {"seg_head.pth", "finetune_config.json"} | ({"adapter_config.json", "adapter_model.safetensors"} if rank else set())
    assert want == {p.name for p in out.iterdir()}
    cfg = json.loads((out / "finetune_config.json").read_text())
    assert cfg["task"] == "segmentation" and cfg["rank"] == rank and cfg["train_samples"] == 36 and cfg["val_samples"] == 12
    assert (cfg["ce_weight"], cfg["dice_weight"], cfg["dice_c0"]) == (1.0, 1.0, 0) and len(cfg["best_dice_per_class"]) == 3


def test_reloaded_segmenter_reproduces_the_validation_predictions(first_run, backbone_dir):
    from dinox.segment import load_segmenter, segment
    rank, out, res = first_run
    model = load_segmenter(backbone_dir, out, DEV)
    assert not any(p.requires_grad for p in model.parameters()) and not model.training
    ds = res["val_dataset"]
    with torch.autocast("cuda", dtype=torch.bfloat16):      # the run validated under bf16 autocast
        for i in range(len(ds)):
            sx, sy, sz = ds.spacings[i].tolist()
            got = segment(model, ds.images[i, 0].numpy(), (sx, sy), sz, input_format="windowed_float")
            assert got.dtype == np.uint8 and got.shape == (32, 32)
            assert np.array_equal(got, res["val_pred"][i].numpy()), f"image {i}"


def test_same_seed_same_head(first_run, backbone_dir, tmp_path):
    rank, out, _ = first_run
    _run(_script(), backbone_dir, tmp_path, rank)
    a, b = torch.load(out / "seg_head.pth", weights_only=True), torch.load(tmp_path / "seg_head.pth", weights_only=True)
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


def test_zz_report_error_to_bound_ratios():
    """Not a check of its own: prints the largest error / bound ratio every test above saw (each was asserted <= 1 there)."""
    for k in sorted(RATIOS):
        print(f"segloss error/bound  {k:24s} {RATIOS[k]:.4f}")
