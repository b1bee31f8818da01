"""MAE objective, host side: the float64 oracle of the masked-token kernels against what the reference's random_masking, decoder
un-shuffle and patchify / forward_loss + autograd recorded (tests/golden/mae_parts.npz), the model's parameter layout against the
reference's (mae_step_tiny.npz), the C ABI's argument checks and the engine's hyper-parameters.  No kernel is launched."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_golden

import _mae_oracle as MO

CASES = ["s16", "s196", "p14"]


@pytest.fixture(scope="module")
def gold():
    return load_golden("mae_parts.npz")


@pytest.fixture(scope="module")
def tiny():
    return load_golden("mae_step_tiny.npz")


def row_err(got, want):
    """max over rows of (max-abs error of the row / max-abs of the reference row); a zero reference row must be matched exactly."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    got, want = got.reshape(-1, got.shape[-1]), want.reshape(-1, want.shape[-1])
    scale, err = np.abs(want).max(1), np.abs(got - want).max(1)
    assert (err[scale == 0] == 0).all()
    return float((err[scale > 0] / scale[scale > 0]).max()) if (scale > 0).any() else 0.0


@pytest.mark.parametrize("tag", CASES)
def test_oracle_matches_reference_fixture(gold, tag):
    """Forward gathers are exact up to the reference's one fp32 add per element (2^-24 relative); the backward sums are at most V
    (tokens) or V (L - Lk) <= 441 (mask token) fp32 adds in the reference: 2e-6 of a row's max-abs covers both; the loss is a mean of
    <= 441 x 588 fp32 terms, 1e-6 relative."""
    V, L, Lk, D, p = (int(v) for v in gold[f"{tag}_dims"])
    assert list(gold["cases"]) == CASES and float(gold["mask_ratio"]) == 0.75 and int(L * (1 - 0.75)) == Lk
    noise = gold[f"{tag}_noise"]
    assert all(len(np.unique(r)) == L for r in noise)
    ids_restore, ids_keep = MO.mask_ids(noise, Lk)
    assert (ids_restore == gold[f"{tag}_ids_restore"]).all()
    assert ((ids_restore >= Lk).astype(np.float32) == gold[f"{tag}_mask"]).all()
    kept = np.take_along_axis(gold[f"{tag}_patches"], ids_keep.astype(np.int64)[:, :, None], axis=1)
    tok = MO.tokens_fwd(kept, gold[f"{tag}_cls"], gold[f"{tag}_pos"][0], ids_keep)
    assert row_err(tok, gold[f"{tag}_tok"]) <= 2e-7
    dpatches, dcls, dpos = MO.tokens_bwd(gold[f"{tag}_gtok"], ids_restore, Lk)
    want_dp = gold[f"{tag}_dpatches"]
    assert row_err(dpatches, np.take_along_axis(want_dp, ids_keep.astype(np.int64)[:, :, None], axis=1)) == 0.0
    assert (want_dp[ids_restore >= Lk] == 0).all()                       # removed patches get no gradient
    assert row_err(dcls[None], gold[f"{tag}_dcls"][0]) <= 2e-6 and row_err(dpos, gold[f"{tag}_dpos"][0]) <= 2e-6
    xd = MO.unshuffle_fwd(gold[f"{tag}_e"], gold[f"{tag}_mask_token"], gold[f"{tag}_dec_pos"][0], ids_restore)
    assert row_err(xd[:, 1:], gold[f"{tag}_xd"]) <= 2e-7                  # (the reference drops the CLS row)
    g = np.concatenate([np.zeros((V, 1, D), np.float32), gold[f"{tag}_gxd"]], axis=1)
    de, dmask = MO.unshuffle_bwd(g, ids_keep, ids_restore)
    assert row_err(de, gold[f"{tag}_de"]) == 0.0 and row_err(dmask[None], gold[f"{tag}_dmask_token"][0]) <= 2e-6
    loss = MO.loss_fwd(gold[f"{tag}_pred"], gold[f"{tag}_imgs"], ids_restore, Lk, p)
    want = float(gold[f"{tag}_loss"])
    assert abs(loss - want) <= 1e-6 * abs(want)
    dpred = MO.loss_bwd(gold[f"{tag}_pred"], gold[f"{tag}_imgs"], ids_restore, Lk, p, float(gold[f"{tag}_gscale"]))
    assert row_err(dpred, gold[f"{tag}_dpred"]) <= 2e-6
    assert (dpred[ids_restore < Lk] == 0).all()


def test_oracle_ties_resolve_as_a_stable_sort():
    noise = np.floor(np.random.default_rng(3).uniform(0, 8, size=(4, 50))).astype(np.float32) / 8
    ids_restore, ids_keep = MO.mask_ids(noise, 12)
    order = torch.argsort(torch.from_numpy(noise), dim=1, stable=True)
    assert (torch.argsort(order, dim=1).numpy() == ids_restore).all() and (order[:, :12].numpy() == ids_keep).all()


def test_oracle_unfold_orders():
    """gather_unfold follows dinox_patch_unfold's column order (c, py, px); the loss target the reference's patchify order (py, px, c)."""
    x = np.arange(2 * 3 * 8 * 8, dtype=np.float64).reshape(2, 3, 8, 8)
    u, tgt = MO.unfold(x, 4), MO.patchify(x, 4)
    assert u[1, 3, 2 * 16 + 1 * 4 + 3] == x[1, 2, 4 + 1, 4 + 3] and tgt[1, 3, (1 * 4 + 3) * 3 + 2] == x[1, 2, 4 + 1, 4 + 3]
    assert MO.unfold(x, 4, ld=64)[:, :, 48:].sum() == 0
    ids = np.array([[3, 0], [1, 2]])
    assert (MO.gather_unfold(x, ids, 4) == np.stack([u[0, 3], u[0, 0], u[1, 1], u[1, 2]])).all()


def _tiny_model(tiny):
    import zoo.arch as arch
    from dinox.mae import MaeModel
    img, patch, dim, depth, heads, regs, scale, ddim, ddepth, dheads = (int(v) for v in tiny["cfg"])
    enc = arch.PatchViT(img_size=img, patch=patch, dim=dim, depth=depth, heads=heads, num_registers=regs, scale_aware=bool(scale))
    return MaeModel(enc, decoder_dim=ddim, mask_ratio=float(tiny["hp"][5]), decoder_depth=ddepth, decoder_heads=dheads)


def test_model_layout_matches_the_reference(tiny):
    """Parameter names, order and shapes are the reference's; so is the fixed sin-cos table, to the bit; the state dict loads the
    reference's tensors; decoder_pos_embed is a parameter that takes no gradient."""
    model = _tiny_model(tiny)
    names = [n for n, _ in model.named_parameters()]
    assert names == list(tiny["param_order"])
    assert ["x".join(str(d) for d in p.shape) for _, p in model.named_parameters()] == list(tiny["param_shapes"])
    assert sum(p.numel() for p in model.parameters()) == int(tiny["n_params"]) == 66400
    assert not model.decoder.decoder_pos_embed.requires_grad and "decoder.decoder_pos_embed" in model.state_dict()
    assert torch.equal(model.decoder.decoder_pos_embed.detach(), torch.from_numpy(tiny["init/decoder.decoder_pos_embed"]))
    init = {k[5:]: torch.from_numpy(v.astype(np.float32)) for k, v in tiny.items() if k.startswith("init/")}
    assert set(init) == set(model.state_dict())
    model.load_state_dict(init)
    assert set(tiny["grad_none"]) == {"encoder.registers", "decoder.decoder_pos_embed"} | {n for n in names if "scale_embed" in n}


def test_reference_defaults_and_decoder_spec():
    import inspect
    from dinox import mae
    sig = inspect.signature(mae.MaeDecoder.__init__).parameters
    assert [sig[k].default for k in ("decoder_dim", "decoder_depth", "decoder_heads", "mlp_ratio")] == [512, 8, 16, 4.0]
    sig = inspect.signature(mae.MaeModel.__init__).parameters
    assert list(sig)[1:4] == ["encoder", "decoder_dim", "mask_ratio"] and sig["decoder_dim"].default == 512 and sig["mask_ratio"].default == 0.75
    assert mae.parse_decoder_spec("512x8x16") == (512, 8, 16) and mae.parse_decoder_spec("32X2X4") == (32, 2, 4)
    for bad in ("512", "512x8", "ax8x16", "512x0x16", "510x8x16", "512x8x7", "512x8x16x2"):
        with pytest.raises(ValueError, match="--mae-decoder"):
            mae.parse_decoder_spec(bad)
    t = mae.sincos_table(16, 3)
    assert t.shape == (1, 10, 16) and float(t[0, 0].abs().max()) == 0 and float(t[0, 1, 4]) == 1.0      # cos(0) of the first patch


def test_export_encoder_round_trips_into_patchvit(tiny):
    import zoo.arch as arch
    from dinox.mae import export_encoder
    model = _tiny_model(tiny)
    sd = export_encoder(model.state_dict())
    assert all(not k.startswith(("encoder.", "decoder.")) for k in sd)
    vit = arch.PatchViT(img_size=32, patch=8, dim=32, depth=2, heads=2, num_registers=2, scale_aware=True)
    vit.load_state_dict(sd)
    assert all(torch.equal(v, model.encoder.state_dict()[k]) for k, v in vit.state_dict().items())
    with pytest.raises(ValueError, match="encoder"):
        export_encoder({"backbone.x": torch.zeros(1)})


def test_step_hyperparameters_gain_the_mae_fields_and_keep_their_defaults():
    from dinox.engine import StepHyperParams
    hp = StepHyperParams()
    assert hp.loss_type == "dino" and hp.simclr_temp == 0.1 and hp.mae_mask_ratio == 0.75
    assert (hp.lr, hp.min_lr, hp.warmup_steps, hp.weight_decay, hp.ema, hp.gram_weight, hp.koleo_weight) == (1e-4, 1e-6, 2500, 0.04, 0.996, 1.0, 0.0)


def test_abi_rejects_bad_arguments_without_a_launch():
    """The checks run on the host, ahead of the launch: the pointers below are never dereferenced."""
    from dinox import _lib
    lib = _lib.lib
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    E = -1
    for V, L, Lk in ((0, 16, 4), (2, 1, 1), (2, 16, 0), (2, 16, 16), (2, 4097, 4)):
        assert lib.dinox_mae_mask_ids(p, p, p, V, L, Lk, None) == E and "Lk=" in _lib.last_error()
        assert lib.dinox_mae_tokens_fwd(p, p, p, p, p, V, L, Lk, 8, 0, None) == E
        assert lib.dinox_mae_tokens_bwd(p, p, p, p, p, V, L, Lk, 8, 0, None) == E
        assert lib.dinox_mae_unshuffle_fwd(p, p, p, p, p, V, L, Lk, 8, 0, None) == E
        assert lib.dinox_mae_unshuffle_bwd(p, p, p, p, p, p, V, L, Lk, 8, 0, None) == E
    assert lib.dinox_mae_mask_ids(None, p, p, 2, 16, 4, None) == E and "null" in _lib.last_error()
    assert lib.dinox_mae_tokens_fwd(p, p, p, p, p, 2, 16, 4, 0, 0, None) == E and "D=" in _lib.last_error()
    assert lib.dinox_mae_tokens_fwd(p, p, p, p, p, 2, 16, 4, 8, 7, None) == E and "dtype" in _lib.last_error()
    assert lib.dinox_mae_gather_unfold(p, p, p, 2, 16, 15, 4, 4, 48, 0, None) == E and "patch" in _lib.last_error()      # W % patch != 0
    assert lib.dinox_mae_gather_unfold(p, p, p, 2, 16, 16, 4, 4, 47, 0, None) == E                                          # ld < 3 p^2
    assert lib.dinox_mae_gather_unfold(p, None, p, 2, 16, 16, 4, 4, 48, 0, None) == E and "null" in _lib.last_error()
    assert lib.dinox_mae_loss_fwd(p, p, p, p, p, 2, 128, 128, 64, 1, 0, 0, None) == E and "patch" in _lib.last_error()       # patch > 32
    assert lib.dinox_mae_loss_fwd(p, p, p, p, p, 2, 16, 16, 4, 4, 2, 0, None) == E and "lead" in _lib.last_error()
    assert lib.dinox_mae_loss_bwd(p, p, p, p, 1.0, 2, 16, 16, 4, 4, 0, 0, 0, None) == E and "alias" in _lib.last_error()
    assert lib.dinox_mae_loss_bwd(p, p, p, p + 128, 1.0, 2, 16, 16, 4, 16, 0, 0, 0, None) == E and "Lk=" in _lib.last_error()


def test_ops_reject_cpu_tensors():
    from dinox import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mae_mask_ids(torch.rand(2, 16), 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mae_loss_fwd(torch.randn(2, 16, 48), torch.randn(2, 3, 16, 16), torch.zeros(2, 16, dtype=torch.int32), 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mae_gather_unfold(torch.randn(2, 3, 16, 16), torch.zeros(2, 4, dtype=torch.int32), 4, torch.float32)
    for name in ("mae_mask_ids", "mae_gather_unfold", "MaeTokensFn", "MaeUnshuffleFn", "MaeLossFn", "mae_loss_fwd", "mae_loss_bwd"):
        assert hasattr(ops, name)


def test_cli_argument_checks_run_before_any_device_work(cli, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the argument check must run before any device work")
    monkeypatch.setattr(cli, "init_process_group", boom)
    monkeypatch.setattr(cli, "detect_hardware", boom)
    with pytest.raises(SystemExit, match="mae is not wired.*--mae-decoder"):
        cli.main(["--loss-type", "mae", "--synthetic", "8"])
    with pytest.raises(SystemExit, match="--mae-decoder takes DIMxDEPTHxHEADS"):
        cli.main(["--loss-type", "mae", "--mae-decoder", "512x8", "--synthetic", "8"])
    with pytest.raises(SystemExit, match="mae.*--local-crops"):
        cli.main(["--loss-type", "mae", "--mae-decoder", "32x2x4", "--local-crops", "2", "--gpu-views", "--synthetic", "8"])
    with pytest.raises(SystemExit, match="mae.*--hip-graph"):
        cli.main(["--loss-type", "mae", "--mae-decoder", "32x2x4", "--hip-graph", "--synthetic", "8"])
    args = cli.parse_cli(["--loss-type", "mae", "--mae-decoder", "32x2x4"])
    assert args.mae_mask_ratio == 0.75 and args.mae_decoder == "32x2x4"
    assert {s for a in cli.build_mae_parser()._actions for s in a.option_strings} == {"--mae-decoder", "--mae-mask-ratio"}
    cli.check_loss_type(args, world=1)
    with pytest.raises(SystemExit, match="mae.*one GPU only"):
        cli.check_loss_type(args, world=2)
    assert cli.MaeModel.__module__ == "dinox.mae" and cli.MaeDecoder.__module__ == "dinox.mae"


# ------------------------------------------------------------------------------------------ the tiny step on the oracle
class _OracleTokens(torch.autograd.Function):
    @staticmethod
    def forward(ctx, patches, cls, pos, ids_restore, ids_keep):
        ctx.ids, ctx.lk = ids_restore, ids_keep.shape[1]
        return torch.from_numpy(MO.tokens_fwd(patches.numpy(), cls.numpy().reshape(-1), pos.numpy()[0], ids_keep))

    @staticmethod
    def backward(ctx, g):
        dp, dcls, dpos = MO.tokens_bwd(g.numpy(), ctx.ids, ctx.lk)
        return torch.from_numpy(dp), torch.from_numpy(dcls).view(1, 1, -1), torch.from_numpy(dpos)[None], None, None


class _OracleUnshuffle(torch.autograd.Function):
    @staticmethod
    def forward(ctx, e, mask_token, dec_pos, ids_restore, ids_keep):
        ctx.ids = (ids_keep, ids_restore)
        return torch.from_numpy(MO.unshuffle_fwd(e.numpy(), mask_token.numpy().reshape(-1), dec_pos.numpy()[0], ids_restore))

    @staticmethod
    def backward(ctx, g):
        de, dmask = MO.unshuffle_bwd(g.numpy(), *ctx.ids)
        return torch.from_numpy(de), torch.from_numpy(dmask).view(1, 1, -1), None, None, None


class _OracleLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, imgs, ids_restore, len_keep, p):
        ctx.args = (pred.numpy().copy(), imgs, ids_restore, len_keep, p)
        return torch.tensor(MO.loss_fwd(*ctx.args), dtype=torch.float64)

    @staticmethod
    def backward(ctx, g):
        return torch.from_numpy(MO.loss_bwd(*ctx.args, gscale=float(g))), None, None, None, None


def _block64(t, w, prefix, heads):
    """A pre-norm transformer block in float64 torch ops: LayerNorm (eps 1e-5), packed qkv [.., 3, h, d], softmax(q k^T / sqrt(d)) v,
    proj, residual; LayerNorm, fc1, exact-erf GELU, fc2, residual."""
    F = torch.nn.functional
    b, n, d = t.shape
    y = F.layer_norm(t, (d,), w[prefix + "norm1.weight"], w[prefix + "norm1.bias"], 1e-5)
    q, k, v = F.linear(y, w[prefix + "attn.qkv.weight"], w[prefix + "attn.qkv.bias"]).view(b, n, 3, heads, d // heads).permute(2, 0, 3, 1, 4)
    a = torch.softmax(q @ k.transpose(-1, -2) / (d // heads) ** 0.5, dim=-1) @ v
    t = t + F.linear(a.transpose(1, 2).reshape(b, n, d), w[prefix + "attn.proj.weight"], w[prefix + "attn.proj.bias"])
    y = F.layer_norm(t, (d,), w[prefix + "norm2.weight"], w[prefix + "norm2.bias"], 1e-5)
    y = F.gelu(F.linear(y, w[prefix + "mlp.fc1.weight"], w[prefix + "mlp.fc1.bias"]))
    return t + F.linear(y, w[prefix + "mlp.fc2.weight"], w[prefix + "mlp.fc2.bias"])


def test_oracle_driven_tiny_step_matches_the_reference_step(tiny):
    """Step 0 of the step fixture, restated without any kernel: the float64 oracle for mask ids, gather + unfold, tokens, un-shuffle and
    the loss (forward and backward, chained by hand), float64 torch ops for the products, LayerNorms and blocks between them.  The loss
    and every gradient the reference recorded agree within 1e-5 (of the tensor's max-abs): the reference ran in fp32, whose round-off
    over these 32-wide sums is ~1e-6.  The parameters the reference left without a gradient get none here either."""
    g = tiny
    F = torch.nn.functional
    img, patch, dim, depth, heads, regs, scale, ddim, ddepth, dheads = (int(v) for v in g["cfg"])
    L = (img // patch) ** 2
    Lk = int(L * (1 - float(g["hp"][5])))
    w = {str(n): torch.from_numpy(g[f"init/{n}"].astype(np.float64)).requires_grad_(True) for n in g["param_order"]}
    imgs = g["batch0"].astype(np.float64)
    ids_restore, ids_keep = MO.mask_ids(g["noise0"], Lk)
    assert ((ids_restore >= Lk) == (g["mask0"] > 0)).all()
    u = torch.from_numpy(MO.gather_unfold(imgs, ids_keep, patch))                       # [V Lk, 3 p^2], column c p p + py p + px
    patches = F.linear(u, w["encoder.patch_embed.weight"].reshape(dim, -1), w["encoder.patch_embed.bias"]).view(-1, Lk, dim)
    t = _OracleTokens.apply(patches, w["encoder.cls_token"], w["encoder.pos_embed"], ids_restore, ids_keep)
    for i in range(depth):
        t = _block64(t, w, f"encoder.blocks.{i}.", heads)
    t = F.layer_norm(t, (dim,), w["encoder.norm.weight"], w["encoder.norm.bias"], 1e-5)
    e = F.linear(t, w["decoder.decoder_embed.weight"], w["decoder.decoder_embed.bias"])
    t = _OracleUnshuffle.apply(e, w["decoder.mask_token"], w["decoder.decoder_pos_embed"].detach(), ids_restore, ids_keep)
    for i in range(ddepth):
        t = _block64(t, w, f"decoder.blocks.{i}.", dheads)
    t = F.layer_norm(t, (ddim,), w["decoder.decoder_norm.weight"], w["decoder.decoder_norm.bias"], 1e-5)
    pred = F.linear(t, w["decoder.decoder_pred.weight"], w["decoder.decoder_pred.bias"])[:, 1:]
    loss = _OracleLoss.apply(pred, imgs, ids_restore, Lk, patch)
    loss.backward()
    assert float(loss.detach()) == pytest.approx(float(g["losses"][0]), rel=1e-5)
    none = {str(n) for n in g["grad_none"]}
    assert {n for n, p in w.items() if p.grad is None} == none
    worst = (0.0, "")
    for n, p in w.items():
        if n in none:
            continue
        want = g[f"grad0/{n}"].astype(np.float64)
        err, scale = float(np.abs(p.grad.numpy() - want).max()), float(np.abs(want).max())
        worst = max(worst, (err / max(scale, 1e-300), n))
        assert err <= 1e-5 * scale, (n, err, scale)
    print(f"oracle step 0: loss {float(loss.detach()):.8f} (reference {float(g['losses'][0]):.8f}); worst gradient error {worst[0]:.2e} of max-abs at {worst[1]}")
    total = float(np.sqrt(sum(float((p.grad ** 2).sum()) for n, p in w.items() if n not in none)))
    assert total == pytest.approx(float(g["grad_norms_all"][0]), rel=1e-5)
