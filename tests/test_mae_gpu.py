"""MAE objective on the device: the masked-token kernels against the reference fixture (tests/golden/mae_parts.npz) and the float64
oracle, the engine's ``loss_type="mae"`` step against three steps of the reference loop (mae_step_tiny.npz), the bf16 gate against
the reference's autocast twin, accumulation, the refusals and the CLI with resume."""
import json

import numpy as np
import pytest
import torch

from conftest import load_golden

import _mae_oracle as MO

pytestmark = pytest.mark.gpu

DEV = "cuda"
CASES = ["s16", "s196", "p14"]      # (V, L, Lk, D, p) = (2,16,4,8,4); (3,196,49,40,4): > 64 and > 128 tokens, D % 64 != 0; (2,4,1,8,14): 3 p^2 = 588
AMP_FACTOR = 1.5                     # tests/test_gpu_parity.py: the HIP bf16 step at most 1.5x as far from fp32 as the reference's own autocast step


@pytest.fixture(scope="module")
def dx():
    from dinox import ops
    import zoo.arch as arch
    import dinox._lib as L
    assert L.lib.dinox_device_ok() == 1, L.last_error()
    return ops, arch


@pytest.fixture(scope="module")
def gold():
    return load_golden("mae_parts.npz")


@pytest.fixture(scope="module")
def tiny():
    g = load_golden("mae_step_tiny.npz")
    g.update(load_golden("mae_step_tiny_more.npz"))
    return g


@pytest.fixture(scope="module")
def oracle(gold):
    """float64 oracle results per case, computed once."""
    out = {}
    for tag in CASES:
        V, L, Lk, D, p = (int(v) for v in gold[f"{tag}_dims"])
        ids_restore, ids_keep = MO.mask_ids(gold[f"{tag}_noise"], Lk)
        kept = np.take_along_axis(gold[f"{tag}_patches"], ids_keep.astype(np.int64)[:, :, None], axis=1)
        g_full = np.random.default_rng(5).standard_normal((V, 1 + L, D)).astype(np.float32)
        out[tag] = dict(dims=(V, L, Lk, D, p), ids_restore=ids_restore, ids_keep=ids_keep, kept=kept, g_full=g_full,
                        tokens_bwd=MO.tokens_bwd(gold[f"{tag}_gtok"], ids_restore, Lk),
                        unshuffle_bwd=MO.unshuffle_bwd(g_full, ids_keep, ids_restore),
                        loss=MO.loss_fwd(gold[f"{tag}_pred"], gold[f"{tag}_imgs"], ids_restore, Lk, p),
                        dpred=MO.loss_bwd(gold[f"{tag}_pred"], gold[f"{tag}_imgs"], ids_restore, Lk, p, 1.0))
    return out


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def row_err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    got, want = got.reshape(-1, got.shape[-1]), want.reshape(-1, want.shape[-1])
    scale, err = np.abs(want).max(1), np.abs(got - want).max(1)
    zero = scale == 0
    assert (err[zero] == 0).all()
    return float((err[~zero] / scale[~zero]).max()) if (~zero).any() else 0.0


# ------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("tag", CASES)
def test_mask_ids_equal_stable_argsort(dx, gold, oracle, tag):
    ops, _ = dx
    V, L, Lk, D, p = oracle[tag]["dims"]
    ids_restore, ids_keep = ops.mae_mask_ids(dev(gold[f"{tag}_noise"]), Lk)
    assert (ids_restore.cpu().numpy() == gold[f"{tag}_ids_restore"]).all() and (ids_keep.cpu().numpy() == oracle[tag]["ids_keep"]).all()


def test_mask_ids_resolve_ties_as_a_stable_sort(dx):
    ops, _ = dx
    noise = torch.floor(torch.rand(5, 196, generator=torch.Generator().manual_seed(3)) * 8) / 8      # 8 levels: ~24 ties per value
    noise[0, :7] = torch.tensor([0.0, -0.0, float("inf"), float("nan"), -1.0, float("nan"), 0.0])
    order = torch.argsort(noise, dim=1, stable=True)
    ids_restore, ids_keep = ops.mae_mask_ids(noise.to(DEV), 49)
    assert torch.equal(ids_restore.cpu().long(), torch.argsort(order, dim=1)) and torch.equal(ids_keep.cpu().long(), order[:, :49])


@pytest.mark.parametrize("tag", CASES)
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_gather_unfold_is_bit_equal_to_rows_of_patch_unfold(dx, gold, oracle, tag, dt):
    ops, _ = dx
    V, L, Lk, D, p = oracle[tag]["dims"]
    x = dev(gold[f"{tag}_imgs"])
    ids_keep = dev(oracle[tag]["ids_keep"])
    u = ops.mae_gather_unfold(x, ids_keep, p, dt)
    full = ops.patch_unfold(x, p, dt)
    rows = (torch.arange(V, device=DEV)[:, None] * L + ids_keep.long()).reshape(-1)
    assert u.shape == (V * Lk, ops.patch_cols(p, dt)) and torch.equal(u, full[rows])
    if dt == torch.float32:
        assert (u.cpu().numpy() == MO.gather_unfold(gold[f"{tag}_imgs"], oracle[tag]["ids_keep"], p).astype(np.float32)).all()


@pytest.mark.parametrize("tag", CASES)
def test_tokens_forward_and_backward(dx, gold, oracle, tag):
    """Forward: one fp32 add per element, bit-equal to the NumPy fp32 expression and to the reference.  Backward: dpatches a copy,
    dcls / dpos sums of at most V <= 3 terms: 1e-5 of the row's max-abs against the float64 oracle and the reference."""
    from dinox import _lib
    ops, _ = dx
    o = oracle[tag]
    V, L, Lk, D, p = o["dims"]
    kept, cls, pos = o["kept"], gold[f"{tag}_cls"], gold[f"{tag}_pos"]
    want = np.concatenate([np.broadcast_to(cls[0] + pos[0, :1], (V, 1, D)), kept + pos[0][1 + o["ids_keep"].astype(np.int64)]], axis=1)
    tok = torch.full((V, 1 + Lk, D), 7.0, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    keep = (dev(kept), dev(cls), dev(pos), dev(o["ids_keep"]))
    assert _lib.lib.dinox_mae_tokens_fwd(keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), keep[3].data_ptr(), tok.data_ptr(),
                                         V, L, L, D, 0, st) == -1                                       # Lk = L: refused, nothing launched
    torch.cuda.synchronize()
    assert bool((tok == 7.0).all())
    assert _lib.lib.dinox_mae_tokens_fwd(keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), keep[3].data_ptr(), tok.data_ptr(),
                                         V, L, Lk, D, 0, st) == 0
    assert (tok.cpu().numpy() == want).all() and (want == gold[f"{tag}_tok"]).all()
    gtok = dev(gold[f"{tag}_gtok"])
    dpatches = torch.empty((V * Lk, D), device=DEV)
    dcls, dpos = torch.empty(D, device=DEV), torch.empty((1 + L, D), device=DEV)
    runs = []
    for _ in range(2):
        assert _lib.lib.dinox_mae_tokens_bwd(gtok.data_ptr(), dev(o["ids_restore"]).data_ptr(), dpatches.data_ptr(), dcls.data_ptr(),
                                             dpos.data_ptr(), V, L, Lk, D, 0, st) == 0
        runs.append((dpatches.clone(), dcls.clone(), dpos.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    o_dp, o_dcls, o_dpos = o["tokens_bwd"]
    assert (dpatches.cpu().numpy().reshape(V, Lk, D) == o_dp.astype(np.float32)).all()
    for want_cls, want_pos in ((o_dcls, o_dpos), (gold[f"{tag}_dcls"].reshape(-1), gold[f"{tag}_dpos"][0])):
        assert row_err(dcls.cpu().numpy()[None], want_cls[None]) <= 1e-5 and row_err(dpos.cpu().numpy(), want_pos) <= 1e-5


@pytest.mark.parametrize("tag", CASES)
def test_tokens_bf16_operand(dx, gold, oracle, tag):
    """dtype code 1: the patch rows arrive in bf16 and are widened exactly before the one fp32 add (bit-equal to the fp32 expression on
    the widened values); dpatches leaves in bf16, the round-to-nearest-even image of the fp32 row; dcls / dpos are those of the fp32 mode."""
    from dinox import _lib
    ops, _ = dx
    o = oracle[tag]
    V, L, Lk, D, p = o["dims"]
    st = torch.cuda.current_stream().cuda_stream
    kept16 = dev(o["kept"]).to(torch.bfloat16)
    cls, pos, ids_keep, ids_restore = dev(gold[f"{tag}_cls"]), dev(gold[f"{tag}_pos"]), dev(o["ids_keep"]), dev(o["ids_restore"])
    tok = torch.full((V, 1 + Lk, D), 7.0, device=DEV)
    assert _lib.lib.dinox_mae_tokens_fwd(kept16.data_ptr(), cls.data_ptr(), pos.data_ptr(), ids_keep.data_ptr(), tok.data_ptr(),
                                         V, L, Lk, D, 1, st) == 0
    want = MO.tokens_fwd(kept16.float().cpu().numpy(), gold[f"{tag}_cls"].reshape(-1), gold[f"{tag}_pos"][0], o["ids_keep"])
    assert (tok.cpu().numpy() == want.astype(np.float32)).all()      # (an fp32 sum of two fp32 values: float64 then one rounding is the same)
    gtok = dev(gold[f"{tag}_gtok"])
    dp16 = torch.full((V * Lk, D), 7.0, dtype=torch.bfloat16, device=DEV)
    dp32 = torch.empty((V * Lk, D), device=DEV)
    dcls, dpos, dcls32, dpos32 = (torch.empty(s, device=DEV) for s in ((D,), (1 + L, D), (D,), (1 + L, D)))
    assert _lib.lib.dinox_mae_tokens_bwd(gtok.data_ptr(), ids_restore.data_ptr(), dp16.data_ptr(), dcls.data_ptr(), dpos.data_ptr(),
                                         V, L, Lk, D, 1, st) == 0
    assert _lib.lib.dinox_mae_tokens_bwd(gtok.data_ptr(), ids_restore.data_ptr(), dp32.data_ptr(), dcls32.data_ptr(), dpos32.data_ptr(),
                                         V, L, Lk, D, 0, st) == 0
    assert torch.equal(dp16, gtok[:, 1:].reshape(V * Lk, D).to(torch.bfloat16))
    assert torch.equal(dcls, dcls32) and torch.equal(dpos, dpos32)


@pytest.mark.parametrize("tag", CASES)
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_unshuffle_forward_and_backward(dx, gold, oracle, tag, dt):
    """Forward bit-equal to the fp32 NumPy expression on the (possibly bf16-rounded) input; backward: de a gather (exact, rounded
    to dt), dmask_token two fixed-order chains of L - Lk <= 147 and V <= 3 fp32 adds: 1e-5 of its max-abs against float64."""
    ops, _ = dx
    o = oracle[tag]
    V, L, Lk, D, p = o["dims"]
    e = dev(gold[f"{tag}_e"], dt)
    mt = dev(gold[f"{tag}_mask_token"]).requires_grad_(True)
    dp = dev(gold[f"{tag}_dec_pos"])
    e_ = e.clone().requires_grad_(True)
    xd = ops.MaeUnshuffleFn.apply(e_, mt, dp, dev(o["ids_restore"]), dev(o["ids_keep"]))
    e32 = e.float().cpu().numpy()
    want = np.empty((V, 1 + L, D), np.float32)
    want[:, 0] = e32[:, 0]
    for v in range(V):
        for q in range(L):
            r = o["ids_restore"][v, q]
            want[v, 1 + q] = e32[v, 1 + r] if r < Lk else gold[f"{tag}_mask_token"].reshape(-1)
    want = want + gold[f"{tag}_dec_pos"]
    assert (xd.detach().cpu().numpy() == want).all()
    if dt == torch.float32:
        assert (want[:, 1:] == gold[f"{tag}_xd"]).all()
    g = dev(o["g_full"])
    xd.backward(g)
    o_de, o_dm = o["unshuffle_bwd"]
    assert torch.equal(e_.grad, dev(o_de.astype(np.float32)).to(dt)) and e_.grad.dtype == dt
    assert row_err(mt.grad.cpu().numpy().reshape(1, -1), o_dm[None]) <= 1e-5
    if dt == torch.float32:       # the reference's gradients under ITS upstream gradient (zero on the CLS row, which it drops)
        e2, mt2 = e.clone().requires_grad_(True), mt.detach().clone().requires_grad_(True)
        xd2 = ops.MaeUnshuffleFn.apply(e2, mt2, dp, dev(o["ids_restore"]), dev(o["ids_keep"]))
        xd2.backward(dev(np.concatenate([np.zeros((V, 1, D), np.float32), gold[f"{tag}_gxd"]], axis=1)))
        assert (e2.grad.cpu().numpy() == gold[f"{tag}_de"]).all()
        assert row_err(mt2.grad.cpu().numpy().reshape(1, -1), gold[f"{tag}_dmask_token"].reshape(1, -1)) <= 1e-5


@pytest.mark.parametrize("tag", CASES)
@pytest.mark.parametrize("lead", [0, 1])
def test_loss_and_its_gradient(dx, gold, oracle, tag, lead):
    """Loss within 1e-5 relative and every dpred row within 1e-5 of its max-abs, against the float64 oracle and the reference (per patch
    a fixed tree over 3 p^2 <= 588 fp32 terms, then one over V L <= 588 patch means); dpred exactly 0 on kept patches and on the CLS row;
    gscale scales the gradient and nothing else; two runs are bit-identical; a bf16 gradient is the rounded fp32 one."""
    ops, _ = dx
    o = oracle[tag]
    V, L, Lk, D, p = o["dims"]
    pred = gold[f"{tag}_pred"]
    if lead:
        pred = np.concatenate([np.full((V, 1, pred.shape[2]), 3.0, np.float32), pred], axis=1)
    x, ids = dev(gold[f"{tag}_imgs"]), dev(o["ids_restore"])
    loss, saved = ops.mae_loss_fwd(dev(pred), x, ids, Lk, p, lead)
    loss2, _ = ops.mae_loss_fwd(dev(pred), x, ids, Lk, p, lead)
    d1, dh, d1b = ops.mae_loss_bwd(saved, 1.0), ops.mae_loss_bwd(saved, 0.5), ops.mae_loss_bwd(saved, 1.0)
    assert torch.equal(loss, loss2) and torch.equal(d1, d1b)
    for want in (o["loss"], float(gold[f"{tag}_loss"])):
        print(f"{tag} lead {lead}: loss rel err {abs(float(loss) - want) / want:.2e}")
        assert abs(float(loss) - want) <= 1e-5 * abs(want)
    d1n = d1.cpu().numpy()
    assert (d1n[:, :lead] == 0).all()
    d1n = d1n[:, lead:]
    assert row_err(d1n, o["dpred"]) <= 1e-5 and row_err(d1n * float(gold[f"{tag}_gscale"]), gold[f"{tag}_dpred"]) <= 1e-5
    assert (d1n[o["ids_restore"] < Lk] == 0).all() and (np.abs(d1n[o["ids_restore"] >= Lk]).max(-1) > 0).all()
    assert row_err(dh.cpu().numpy()[:, lead:], 0.5 * o["dpred"]) <= 1e-5
    d16 = ops.mae_loss_bwd(saved, 1.0, out_dtype=torch.bfloat16)
    assert d16.dtype == torch.bfloat16 and torch.equal(d16, d1.to(torch.bfloat16))
    # bf16 predictions: the loss of the rounded values (the oracle on the same rounded input)
    p16 = dev(pred).to(torch.bfloat16)
    l16, _ = ops.mae_loss_fwd(p16, x, ids, Lk, p, lead)
    want16 = MO.loss_fwd(p16.float().cpu().numpy()[:, lead:], gold[f"{tag}_imgs"], o["ids_restore"], Lk, p)
    assert abs(float(l16) - want16) <= 1e-5 * want16


def test_error_paths_leave_outputs_untouched(dx):
    from dinox import _lib
    ops, _ = dx
    lib, st = _lib.lib, torch.cuda.current_stream().cuda_stream
    f = lambda *s: torch.full(s, 7.0, device=DEV)
    i = lambda *s: torch.full(s, 7, dtype=torch.int32, device=DEV)
    noise, ids_r, ids_k = torch.rand(2, 16, device=DEV), i(2, 16), i(2, 4)
    assert lib.dinox_mae_mask_ids(noise.data_ptr(), ids_r.data_ptr(), ids_k.data_ptr(), 2, 16, 16, st) == -1
    x, u = torch.randn(2, 3, 16, 16, device=DEV), f(8, 48)
    assert lib.dinox_mae_gather_unfold(x.data_ptr(), ids_k.data_ptr(), u.data_ptr(), 2, 16, 16, 4, 4, 40, 0, st) == -1
    pred, loss, ws, dpred = torch.randn(2, 16, 48, device=DEV), f(1), f(32), f(2, 16, 48)
    assert lib.dinox_mae_loss_fwd(pred.data_ptr(), x.data_ptr(), ids_r.data_ptr(), loss.data_ptr(), ws.data_ptr(), 2, 16, 16, 4, 0, 0, 0, st) == -1
    assert lib.dinox_mae_loss_bwd(pred.data_ptr(), x.data_ptr(), ids_r.data_ptr(), dpred.data_ptr(), 1.0, 2, 16, 16, 4, 4, 0, 0, 9, st) == -1
    g, de, dm, ws2 = torch.randn(2, 17, 8, device=DEV), f(2, 5, 8), f(8), f(2, 8)
    assert lib.dinox_mae_unshuffle_bwd(g.data_ptr(), ids_k.data_ptr(), ids_r.data_ptr(), de.data_ptr(), dm.data_ptr(), None, 2, 16, 4, 8, 0, st) == -1
    torch.cuda.synchronize()
    for t in (u, loss, ws, dpred, de, dm, ws2):
        assert bool((t == 7.0).all())
    assert bool((ids_r == 7).all()) and bool((ids_k == 7).all())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mae_mask_ids(torch.rand(2, 16), 4)
    with pytest.raises(ValueError, match="int32"):
        ops.mae_loss_fwd(pred, x, ids_r.long(), 4, 4)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_kept_rows_patch_embed_equals_embed_all_then_gather(dx, mode):
    """MaeTokensFn runs the patch-embedding product on M = V*Lk rows (checked through ops.TRACE_KERNELS' sibling, the GemmTimer record);
    its tokens equal TokensFn's rows [0 | 1 + ids_keep] at the project bar (1e-3 of the max-abs; bf16: the bf16 step of the values)."""
    ops, arch = dx
    dt = torch.float32 if mode == "fp32" else torch.bfloat16
    torch.manual_seed(11)
    vit = arch.PatchViT(img_size=56, patch=4, dim=40, depth=1, heads=2, num_registers=0).to(DEV)
    V, L, Lk = 3, 196, 49
    x = torch.randn(V, 3, 56, 56, device=DEV)
    ids_restore, ids_keep = ops.mae_mask_ids(torch.rand(V, L, device=DEV), Lk)
    with ops.compute_dtype(dt), torch.no_grad():
        full = ops.TokensFn.apply(x, vit.patch_embed.weight, vit.patch_embed.bias, vit.cls_token, vit.pos_embed, None, None, 4)
        timer = ops.GemmTimer(every=1)
        with timer:
            tok = ops.MaeTokensFn.apply(x, vit.patch_embed.weight, vit.patch_embed.bias, vit.cls_token, vit.pos_embed, ids_restore, ids_keep, 4)
    shapes = [tuple(int(v) for v in line.split()[1:4]) for line in timer.text.splitlines() if len(line.split()) == 13]
    assert shapes == [(V * Lk, 40, 48)], shapes                           # the one product of the node: M = V*Lk, not V*L
    want = torch.cat([full[:, :1], torch.gather(full[:, 1:], 1, ids_keep.long()[:, :, None].expand(-1, -1, 40))], 1)
    tol = 1e-3 if mode == "fp32" else 2 ** -7
    assert float((tok - want).abs().max()) <= tol * float(want.abs().max())


# ------------------------------------------------------------------------------------------ engine
def _tiny_engine(arch, g, amp=None, accum=1):
    from dinox.engine import StepHyperParams, TrainEngine
    from dinox.mae import MaeModel
    img, patch, dim, depth, heads, regs, scale, ddim, ddepth, dheads = (int(v) for v in g["cfg"])
    enc = arch.PatchViT(img_size=img, patch=patch, dim=dim, depth=depth, heads=heads, num_registers=regs, scale_aware=bool(scale))
    model = MaeModel(enc, decoder_dim=ddim, decoder_depth=ddepth, decoder_heads=dheads)
    model.load_state_dict({k[5:]: torch.from_numpy(v.astype(np.float32)) for k, v in g.items() if k.startswith("init/")})
    lr, min_lr, warmup, max_steps, wd, ratio = (float(v) for v in g["hp"])
    hp = StepHyperParams(lr=lr, min_lr=min_lr, warmup_steps=int(warmup), max_steps=int(max_steps), weight_decay=wd, loss_type="mae",
                         mae_mask_ratio=ratio)
    return TrainEngine(model.to(DEV), None, 64, hp, amp_dtype=amp, accumulation_steps=accum), model


def _grads(model):
    return {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm())


def test_engine_matches_three_reference_steps(dx, tiny):
    """fp32 parity bar of the project (README: 1e-3 rel): loss and grad-norm rel 1e-3, every stored gradient within 1e-3 of its
    tensor's max-abs, the model after step 3 within 1e-3; the never-reached parameters bit-identical to their initial values."""
    _, arch = dx
    g = tiny
    eng, model = _tiny_engine(arch, g)
    none = set(g["grad_none"])
    for step in range(3):
        out = eng.step(dev(g[f"batch{step}"], torch.float32), None, mask_noise=dev(g[f"noise{step}"]))
        assert set(out) == {"loss", "dino", "gram", "koleo", "grad_norm_sq", "lr", "mae"}
        s = eng.scalars()
        print(f"step {step}: loss {s['loss']:.6f} (ref {g['losses'][step]:.6f}) grad_norm {s['grad_norm']:.6f} (ref {g['grad_norms'][step]:.6f})")
        assert s["loss"] == pytest.approx(float(g["losses"][step]), rel=1e-3) and s["mae"] == s["loss"]
        assert s["grad_norm"] == pytest.approx(float(g["grad_norms"][step]), rel=1e-3)
        assert s["lr"] == pytest.approx(float(g["lrs"][step]), rel=1e-12)
        if step != 1:
            got = _grads(model)
            assert set(got) == {n for n in g["param_order"] if n not in none}
            for n, gr in got.items():
                want = torch.from_numpy(g[f"grad{step}/{n}"])
                err, scale = float((gr.cpu() - want).abs().max()), float(want.abs().max())
                assert err <= 1e-3 * scale + 1e-9, (step, n, err, scale)
    # Where the reference's own gradient was numerically zero in some step (|g| < 1e-6: the key biases, which the softmax cancels -- 1 % of
    # the reached elements, recorded by the fixture), Adam's g / sqrt(v) turns round-off into a move of +-lr per step, of round-off sign:
    # those elements are held to 2.1 x the sum of the three learning rates (the rule of tests/test_simclr_gpu.py), all others to 1e-3.
    assert float(g["small_grad_share"]) <= 0.10
    lr_sum = float(sum(float(v) for v in g["lrs"][:3]))
    sd = model.state_dict()
    for n in g["param_order"]:
        want = torch.from_numpy(g[f"student3/{n}"])
        d = (sd[n].cpu() - want).abs()
        m = torch.from_numpy(g[f"small/{n}"]) if n not in none else torch.zeros_like(want, dtype=torch.bool)
        if m.any():
            assert float(d[m].max()) <= 2.1 * lr_sum, (n, float(d[m].max()))
        if (~m).any():
            assert float(d[~m].max()) <= 1e-3 * float(want.abs().max()) + 1e-9, (n, float(d[~m].max()))
    for n in none:
        assert dict(model.named_parameters())[n].grad is None
        assert torch.equal(sd[n].cpu(), torch.from_numpy(g[f"init/{n}"].astype(np.float32))), n


def test_engine_bf16_within_autocast_distance(dx, tiny):
    """relL2(HIP bf16, reference fp32) <= 1.5 x relL2(reference autocast, reference fp32) per gradient tensor (the rule of
    tests/test_gpu_parity.py, restated here), on step 0."""
    _, arch = dx
    g = tiny
    eng, model = _tiny_engine(arch, g, amp=torch.bfloat16, accum=2)      # two micro-steps per update: after the first, the gradients are still there
    eng.step(dev(g["batch0"], torch.float32), None, mask_noise=dev(g["noise0"]))
    got = {n: 2.0 * v for n, v in _grads(model).items()}                  # (gscale = 1/2)
    worst = (0.0, "")
    bad = []
    for n, gr in got.items():
        r32 = torch.from_numpy(g[f"grad0/{n}"])
        if float(r32.abs().max()) <= 1e-6:
            continue
        d_ref, d_hip = rel_l2(g[f"autocast_grad0/{n}"], r32), rel_l2(gr, r32)
        ratio = d_hip / max(d_ref, 1e-12)
        worst = max(worst, (ratio, n))
        if ratio > AMP_FACTOR:
            bad.append((n, d_hip, d_ref))
    print(f"mae tiny bf16: worst (HIP distance / reference-autocast distance) = {worst[0]:.2f} at {worst[1]}")
    # The loss is held to the same factor of the reference's own autocast distance, plus one bf16 half-ulp of the loss (2^-9): the two
    # autocast losses are single numbers whose errors can cancel to nearly nothing, which a sum over thousands of gradient elements cannot,
    # and the prediction the loss reads is stored in bf16, so 2^-9 relative is the resolution of what it is computed from.
    loss, ref, twin = float(eng.last["loss"]), float(g["losses"][0]), float(g["autocast_loss0"])
    print(f"mae tiny bf16: loss {loss:.6f}, reference fp32 {ref:.6f}, reference autocast {twin:.6f}")
    assert abs(loss - ref) <= AMP_FACTOR * abs(twin - ref) + 2.0 ** -9 * ref
    assert not bad, bad


def test_accumulation_over_two_half_batches_equals_one_step(dx, tiny):
    """Both halves remove the same number of patches, so the mean over the full batch is the mean of the two half means."""
    _, arch = dx
    g = tiny
    batch, noise = dev(g["batch0"], torch.float32), dev(g["noise0"])
    e1, m1 = _tiny_engine(arch, g)
    e1.step(batch, None, mask_noise=noise)
    e2, m2 = _tiny_engine(arch, g, accum=2)
    w0 = e2.flat_p.clone()
    o = e2.step(batch[:3], None, mask_noise=noise[:3])
    assert float(o["grad_norm_sq"]) == 0.0 and torch.equal(e2.flat_p, w0)          # no optimiser step after the first micro-batch
    e2.step(batch[3:], None, mask_noise=noise[3:])
    ga, gb = e1.flat_g, e2.flat_g
    assert float((ga - gb).abs().max()) <= 1e-5 * float(ga.abs().max())
    assert e1.opt_steps == e2.opt_steps == 1


def test_engine_refusals(dx, tiny):
    ops, arch = dx
    from dinox.engine import StepHyperParams, TrainEngine
    g = tiny
    eng, model = _tiny_engine(arch, g)
    batch = dev(g["batch0"], torch.float32)
    with pytest.raises(ValueError, match="local crops"):
        eng.step(batch, None, torch.randn(6, 3, 16, 16, device=DEV), None)
    with pytest.raises(ValueError, match="PatchOperand"):
        eng.step(ops.PatchOperand(ops.patch_unfold(batch, 8, torch.float32), 6, 32, 8))
    assert eng.step_count == 0
    hp = StepHyperParams(loss_type="mae")
    with pytest.raises(ValueError, match="loss_type.*MaeModel"):
        TrainEngine(arch.DinoStudentTeacher(model.encoder, 64), None, 64, hp)
    with pytest.raises(ValueError, match="use_graph"):
        TrainEngine(model, None, 64, hp, use_graph=True)
    eng.step(batch, torch.rand(6, 3, device=DEV))                      # spacing is accepted and ignored; the noise comes from torch's generator
    assert np.isfinite(eng.scalars()["loss"])


def test_model_forward_and_forward_loss_agree_with_the_fused_loss(dx, tiny):
    _, arch = dx
    g = tiny
    _, model = _tiny_engine(arch, g)
    batch, noise = dev(g["batch0"], torch.float32), dev(g["noise0"])
    with torch.no_grad():
        pred, mask = model(batch, noise)
        assert pred.shape == (6, 16, 192) and (mask.cpu().numpy() == g["mask0"]).all()
        a, b = model.forward_loss(batch, pred, mask), model.loss(batch, noise)
        c = model.forward_loss(batch, pred, mask.clone())                 # any 0 / 1 mask with the same count per sample
    assert float(a) == float(b) == float(c) and float(a) == pytest.approx(float(g["losses"][0]), rel=1e-3)


# ------------------------------------------------------------------------------------------ CLI
def _same(a, b):
    """Bitwise equality of two checkpoint entries (tensors, numbers, nested dicts / lists of them)."""
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


def test_cli_trains_checkpoints_and_resumes(dx, cli, tmp_path, capsys):
    """Four steps with a checkpoint every two: finite losses of one order of magnitude, both checkpoint entries hold the same MaeModel
    state dict (encoder.* / decoder.*), the optimiser state has no entry for the never-reached parameters.  Then the checkpoints of step
    4 are removed and --resume auto continues from step 2: its final checkpoint (weights, both entries, optimiser moments and step, the
    device generator) equals the uninterrupted run's bitwise, and so do the logged losses of steps 2 and 3."""
    common = ["--loss-type", "mae", "--mae-decoder", "32x2x4", "--synthetic", "64", "--config", "custom", "--vit-patch", "8", "--vit-dim", "32",
              "--vit-depth", "2", "--vit-heads", "2", "--img-size", "32", "--batch-size", "8", "--num-workers", "0", "--monitor-every", "4",
              "--warmup-steps", "2", "--lr", "1e-3", "--ckpt-every", "2", "--scale-aware", "--run-dir", str(tmp_path / "runs"), "--max-steps", "4"]
    log1, log2 = tmp_path / "a.jsonl", tmp_path / "b.jsonl"
    cli.main(common + ["--log-json", str(log1)])
    out = capsys.readouterr().out
    assert "mae_decoder=32x2x4" in out and "checkpoint_saved=" in out and "final_checkpoint=" in out and "monitor_saved=" in out
    rec1 = [json.loads(l) for l in log1.read_text().splitlines()]
    losses = [r["loss"] for r in rec1]
    assert len(losses) == 4 and np.isfinite(losses).all() and max(losses) <= 10 * min(losses)
    run = sorted((tmp_path / "runs").iterdir())[-1]
    payload = torch.load(run / "checkpoint_00000004.pth", map_location="cpu", weights_only=False)
    whole = torch.load(run / "checkpoint_final_00000004.pth", map_location="cpu", weights_only=False)
    keys = set(payload["student"])
    assert {k.split(".")[0] for k in keys} == {"encoder", "decoder"} and "decoder.decoder_pos_embed" in keys
    assert all(torch.equal(payload["student"][k], payload["teacher"][k]) for k in keys)
    first = torch.load(run / "checkpoint_00000002.pth", map_location="cpu", weights_only=False)
    frozen = [k for k in keys if torch.equal(first["student"][k], payload["student"][k])]
    assert set(frozen) == {"encoder.registers", "decoder.decoder_pos_embed"} | {k for k in keys if "scale_embed" in k}
    names = list(payload["student"])                                        # state-dict order = parameters() order here (no buffers)
    assert {names[i] for i in payload["opt"]["state"]} == keys - set(frozen)
    (run / "checkpoint_00000004.pth").unlink()
    (run / "checkpoint_final_00000004.pth").unlink()
    cli.main(common + ["--resume", "auto", "--log-json", str(log2)])
    out = capsys.readouterr().out
    assert "resumed_from_step=2" in out
    after = torch.load(run / "checkpoint_final_00000004.pth", map_location="cpu", weights_only=False)
    assert after["step"] == whole["step"] == 4
    for entry in ("student", "teacher"):
        bad = [k for k in whole[entry] if not _same(whole[entry][k], after[entry][k])]
        assert list(after[entry]) == list(whole[entry]) and not bad, (entry, bad)
    assert _same(whole["opt"], after["opt"]) and int(float(after["opt"]["state"][0]["step"])) == 4
    assert _same(whole["rng"]["cuda"], after["rng"]["cuda"])              # as many mask-noise draws, from the restored state
    assert [json.loads(l) for l in log2.read_text().splitlines()] == rec1[2:]
