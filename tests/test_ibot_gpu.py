"""GPU tests of the iBOT masked-patch objective: the kernels of csrc/ibot.hip against float64 with derived bounds
(tests/_ibot_oracle.py), the engine step against a plain-torch statement of the whole objective, its invariants (empty mask = the
step without the term, bit-reproducible, accumulation, data parallel) and the command line."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import _ibot_oracle as IO
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda"
RATIOS = {}          # kernel -> largest error / bound seen (printed by the last test; DESIGN.md section 4 records them)


@pytest.fixture(scope="module")
def dx():
    from dinox import ops
    import zoo.arch as arch
    import dinox._lib as L
    assert L.lib.dinox_device_ok() == 1, L.last_error()
    return ops, arch


def within(name, got, ref, bound):
    got, ref, bound = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bound, np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert np.isfinite(got).all(), name
    ratio = float((np.abs(got - ref) / bound).max()) if got.size else 0.0
    key = name.split("[")[0]
    RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)
    assert ratio <= 1.0, f"{name}: error / bound = {ratio:.3f}"


def dev_view(a, offset):
    """A device copy of ``a`` whose first element sits ``offset`` floats past a 256-byte boundary."""
    a = np.ascontiguousarray(a, np.float32)
    buf = torch.empty(a.size + 64, dtype=torch.float32, device=DEV)
    v = buf[offset:offset + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    return v


# ------------------------------------------------------------------------------------------ ibot_ce
_CE_REF = {}


def ce_case(regime, M, K):
    """Inputs and float64 reference of one shape, computed once and shared by the aligned and the offset run."""
    key = (regime, M, K)
    if key not in _CE_REF:
        s, t, c = IO.dino_inputs(regime, M, M, K, seed=M + K)
        w = np.random.default_rng(M * K).uniform(0.05, 1.0, M).astype(np.float32)
        if M > 1:
            w[M // 2] = 0.0
        o = IO.ibot_ce(s, t, c, w, 0.1, 0.04, scale=1.0 / 6, grad_scale=0.5)
        _CE_REF[key] = (s, t, c, w, o, IO.bound_ibot(o))
    return _CE_REF[key]


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset"])
@pytest.mark.parametrize("regime", ["normal", "underflow", "onehot"])
@pytest.mark.parametrize("M,K", [(1, 8), (5, 8), (130, 8), (1, 1028), (5, 1028), (130, 1028), (1, 8192), (5, 8192), (130, 8192),
                                 (1, 2052), (5, 2052), (1, 4096), (5, 4096), (1, 4100), (5, 4100), (1, 1030), (5, 1030), (1, 8196), (5, 8196)])
def test_ibot_ce_vs_float64(dx, M, K, regime, offset):
    """Aligned operands with K % 4 == 0 and K <= 8192 run the register-resident kernel, operands one float off the scalar kernel.
    K -> instantiation of the aligned run (K4 = K / 4 float4 groups, NV = ceil(K4 / 256) rounded up to 1, 2, 4, 8): 8 -> <1> with 254 idle
    threads; 1028 -> <2>, ragged (K4 = 257); 2052 -> <4>, ragged (K4 = 513: the third and fourth group hold one float4 and none); 4096 ->
    <4>, full; 4100 -> <8> with K4 = 1025: groups 5, 6 and 7 lie wholly past the row's end, hold -inf and drop out of the output pass;
    8192 -> <8>, full; 1030 -> the scalar kernel on aligned rows (K % 4 != 0); 8196 -> the scalar kernel by size (K > 8192), aligned.
    The offset run of every K is the scalar kernel by alignment."""
    ops, _ = dx
    s, t, c, w, o, b = ce_case(regime, M, K)
    sd, td, cd = dev_view(s, offset), dev_view(t, offset), dev_view(c, offset)
    wd = torch.from_numpy(w).to(DEV)
    ds_buf = dev_view(np.zeros((M, K)), offset)
    loss, ds, row = ops.ibot_ce(sd, td, cd, wd, 0.1, 0.04, scale=1.0 / 6, grad_scale=0.5, ds_out=ds_buf)
    name = f"ibot_ce[{regime},{M}x{K},{'offset' if offset else 'aligned'}]"
    ds, row, loss = ds.cpu().numpy(), row.cpu().numpy(), loss.cpu().numpy()
    within(name.replace("ibot_ce", "ibot_ce.row_loss"), row, o["row"], b["row"] + IO.CE_LOSS_RTOL * np.abs(o["row"]))
    within(name.replace("ibot_ce", "ibot_ce.ds"), ds, o["ds"], b["ds"] + IO.CE_DS_RTOL * np.abs(o["ds"]).max(1, keepdims=True))
    within(name.replace("ibot_ce", "ibot_ce.loss"), loss, [o["loss"]], b["loss"] + IO.CE_LOSS_RTOL * abs(o["loss"]))
    if M > 1:
        assert not ds[M // 2].any()                                                                    # a zero weight: the row's gradient is exactly 0
    loss2, none, row2 = ops.ibot_ce(sd, td, cd, wd, 0.1, 0.04, scale=1.0 / 6, want_grad=False)         # ds = NULL: the same loss, bit for bit
    assert none is None and np.array_equal(loss2.cpu().numpy(), loss) and np.array_equal(row2.cpu().numpy(), row)


@pytest.mark.parametrize("K,offset", [(8192, 0), (1028, 0), (1028, 1), (2052, 0), (8196, 0)])
def test_ibot_ce_does_not_overflow_at_large_logits(dx, K, offset):
    """teacher_temp 0.04 and logits of +-60: (t - c) / tt reaches 1500 and exp of it leaves fp32 (and s / 0.1 = 600 does too); the
    max-shifted kernels stay finite and inside the same bounds."""
    ops, _ = dx
    M = 5
    r = np.random.default_rng(K)
    s, t = r.uniform(-60, 60, (M, K)).astype(np.float32), r.uniform(-60, 60, (M, K)).astype(np.float32)
    c, w = r.uniform(-1, 1, K).astype(np.float32), np.full(M, 0.2, np.float32)
    with np.errstate(over="ignore"):
        assert not np.isfinite(np.exp(np.float32(t.max() / 0.04)))
    o = IO.ibot_ce(s, t, c, w, 0.1, 0.04)
    b = IO.bound_ibot(o)
    loss, ds, row = ops.ibot_ce(dev_view(s, offset), dev_view(t, offset), dev_view(c, offset), torch.from_numpy(w).to(DEV), 0.1, 0.04)
    within("ibot_ce.row_loss[large]", row.cpu().numpy(), o["row"], b["row"] + IO.CE_LOSS_RTOL * np.abs(o["row"]))
    within("ibot_ce.ds[large]", ds.cpu().numpy(), o["ds"], b["ds"] + IO.CE_DS_RTOL * np.abs(o["ds"]).max(1, keepdims=True))
    within("ibot_ce.loss[large]", loss.cpu().numpy(), [o["loss"]], b["loss"] + IO.CE_LOSS_RTOL * abs(o["loss"]))


# ------------------------------------------------------------------------------------------ mask token in and out
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("D", [8, 384])
def test_put_mask_and_its_backward(dx, D, bf16):
    ops, _ = dx
    V, P = 4, 25
    dt = torch.bfloat16 if bf16 else torch.float32
    r = np.random.default_rng(D)
    patches = IO.round_to(r.standard_normal((V * P, D)), bf16)
    token = r.standard_normal(D).astype(np.float32)
    for tag, idx in IO.example_masks(V, P).items():
        pd = torch.from_numpy(patches).to(DEV, dt)
        idx_d = torch.from_numpy(idx).to(DEV)
        ops.ibot_put_mask_(pd, torch.from_numpy(token).to(DEV), idx_d)
        assert np.array_equal(pd.float().cpu().numpy(), IO.put_mask(patches, token, idx, bf16)), tag       # a rounded copy: exact
        g = IO.round_to(r.standard_normal((V * P, D)), bf16)
        gd = torch.from_numpy(g).to(DEV, dt)
        dmask = ops.ibot_put_mask_bwd_(gd, idx_d)
        want, mag, zeroed = IO.put_mask_bwd(g, idx)
        assert dmask.shape == (1, 1, D)
        within(f"put_mask_bwd[{tag}]", dmask.reshape(-1).cpu().numpy(), want, (len(idx) + 2) * IO.U * mag + IO.TINY)
        out = gd.float().cpu().numpy()
        assert np.array_equal(out, zeroed) and not out[idx].any(), tag                                    # exactly 0 there, untouched elsewhere


# ------------------------------------------------------------------------------------------ gather / scatter-add
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("D", [8, 384])
def test_gather_and_scatter_add_rows(dx, D, bf16):
    ops, _ = dx
    dt = torch.bfloat16 if bf16 else torch.float32
    r = np.random.default_rng(D + 1)
    rows, M, row0 = 77, 70, 3
    src = r.standard_normal((rows, D)).astype(np.float32)
    row = np.sort(r.choice(rows, M, replace=False)).astype(np.int32)
    row_d = torch.from_numpy(row).to(DEV)
    out = torch.full((row0 + M + 2, D), 7.0, dtype=dt, device=DEV)
    ops.gather_rows(torch.from_numpy(src).to(DEV), row_d, dt, out=out, out_row0=row0)
    got = out.float().cpu().numpy()
    assert np.array_equal(got[row0:row0 + M], IO.round_to(src[row], bf16))                 # exact in fp32, one rounding in bf16
    assert np.all(got[:row0] == 7.0) and np.all(got[row0 + M:] == 7.0)
    dst = r.standard_normal((rows, D)).astype(np.float32)
    add = IO.round_to(r.standard_normal((row0 + M, D)), bf16)
    dst_d = torch.from_numpy(dst).to(DEV)
    ops.scatter_add_rows_(dst_d, row_d, torch.from_numpy(add).to(DEV, dt), src_row0=row0)
    want = dst.astype(np.float64)
    want[row] += add[row0:row0 + M]
    mag = np.abs(dst.astype(np.float64))
    mag[row] += np.abs(add[row0:row0 + M])
    within("scatter_add_rows", dst_d.cpu().numpy(), want, IO.U * mag + IO.TINY)                 # one rounded add per element
    untouched = np.setdiff1d(np.arange(rows), row)
    assert np.array_equal(dst_d.cpu().numpy()[untouched], dst[untouched])


def test_out_of_range_indices_touch_nothing(dx):
    """Entries outside [0, rows) are skipped, never dereferenced: the operands sit in the middle of a guarded buffer whose canaries on
    either side -- where a negative or a too large row would land -- stay what they were, and so does the operand itself."""
    ops, _ = dx
    rows, D, guard = 10, 8, 40
    bad = torch.tensor([-1, rows, -guard, rows + guard - 1, 2 ** 31 - 1, -2 ** 31], dtype=torch.int32, device=DEV)
    M = bad.numel()

    def guarded():
        buf = torch.full(((rows + 2 * guard), D), 3.0, dtype=torch.float32, device=DEV)
        return buf, buf[guard:guard + rows]
    token = torch.ones(D, device=DEV)
    buf, mid = guarded()
    ops.ibot_put_mask_(mid, token, bad)
    assert bool((buf == 3.0).all())
    buf, mid = guarded()
    dmask = ops.ibot_put_mask_bwd_(mid, bad)
    assert bool((buf == 3.0).all()) and not bool(dmask.any())
    buf, mid = guarded()
    ops.scatter_add_rows_(mid, bad, torch.ones((M, D), device=DEV))
    assert bool((buf == 3.0).all())
    buf, mid = guarded()
    out = torch.full((M, D), 5.0, device=DEV)
    ops.gather_rows(mid, bad, torch.float32, out=out)
    assert bool((out == 5.0).all()) and bool((buf == 3.0).all())


# The four row kernels launch grid_1d(M * D, 256, 4096): with M * D just above 4096 * 256 (and no multiple of it) every workgroup's
# grid-stride loop takes a second, partial trip, which the cases above (M * D <= 30 000) never do.
CAP_M, CAP_D, CAP_ROWS = 4034, 260, 4100


def _cap_case(seed):
    assert 4096 * 256 < CAP_M * CAP_D < 2 * 4096 * 256 and (CAP_M * CAP_D) % (4096 * 256) != 0
    r = np.random.default_rng(seed)
    return r, np.sort(r.choice(CAP_ROWS, CAP_M, replace=False)).astype(np.int32)


def test_gather_rows_past_the_grid_cap(dx):
    ops, _ = dx
    r, row = _cap_case(1)
    src = r.standard_normal((CAP_ROWS, CAP_D)).astype(np.float32)
    out = torch.full((CAP_M + 2, CAP_D), 7.0, device=DEV)
    ops.gather_rows(torch.from_numpy(src).to(DEV), torch.from_numpy(row).to(DEV), torch.float32, out=out, out_row0=1)
    got = out.cpu().numpy()
    assert np.array_equal(got[1:1 + CAP_M], src[row]) and np.all(got[0] == 7.0) and np.all(got[1 + CAP_M] == 7.0)


def test_scatter_add_rows_past_the_grid_cap(dx):
    ops, _ = dx
    r, row = _cap_case(2)
    dst = r.standard_normal((CAP_ROWS, CAP_D)).astype(np.float32)
    add = r.standard_normal((CAP_M, CAP_D)).astype(np.float32)
    dst_d = torch.from_numpy(dst).to(DEV)
    ops.scatter_add_rows_(dst_d, torch.from_numpy(row).to(DEV), torch.from_numpy(add).to(DEV))
    want, mag = dst.astype(np.float64), np.abs(dst.astype(np.float64))
    want[row] += add
    mag[row] += np.abs(add)
    within("scatter_add_rows[cap]", dst_d.cpu().numpy(), want, IO.U * mag + IO.TINY)            # one rounded add per element
    untouched = np.setdiff1d(np.arange(CAP_ROWS), row)
    assert np.array_equal(dst_d.cpu().numpy()[untouched], dst[untouched])


def test_put_mask_past_the_grid_cap(dx):
    ops, _ = dx
    r, idx = _cap_case(3)
    patches = r.standard_normal((CAP_ROWS, CAP_D)).astype(np.float32)
    token = r.standard_normal(CAP_D).astype(np.float32)
    pd = torch.from_numpy(patches).to(DEV)
    ops.ibot_put_mask_(pd, torch.from_numpy(token).to(DEV), torch.from_numpy(idx).to(DEV))
    assert np.array_equal(pd.cpu().numpy(), IO.put_mask(patches, token, idx, False))


def test_put_mask_bwd_past_the_grid_cap(dx):
    ops, _ = dx
    r, idx = _cap_case(4)
    g = r.standard_normal((CAP_ROWS, CAP_D)).astype(np.float32)
    gd = torch.from_numpy(g).to(DEV)
    dmask = ops.ibot_put_mask_bwd_(gd, torch.from_numpy(idx).to(DEV))
    want, mag, zeroed = IO.put_mask_bwd(g, idx)
    within("put_mask_bwd[cap]", dmask.reshape(-1).cpu().numpy(), want, (len(idx) + 2) * IO.U * mag + IO.TINY)
    assert np.array_equal(gd.cpu().numpy(), zeroed)                                              # exactly 0 on the masked rows, untouched elsewhere


def test_entries_reject_bad_arguments_on_the_device(dx):
    """With live device pointers: every invalid argument is DINOX_EINVAL and the outputs keep their fill (nothing was launched)."""
    from dinox import _lib
    L = _lib.lib
    M, K = 4, 8
    s, t, c, w = (torch.ones(n, device=DEV) for n in (M * K, M * K, K, M))
    loss, ds, row = torch.full((1,), 9.0, device=DEV), torch.full((M * K,), 9.0, device=DEV), torch.full((M,), 9.0, device=DEV)
    p = lambda x: x.data_ptr()
    for kw in (dict(M=0), dict(K=0), dict(ts=0.0), dict(tt=0.0)):
        a = dict(M=M, K=K, ts=0.1, tt=0.04)
        a.update(kw)
        assert L.dinox_ibot_ce(p(s), p(t), p(c), p(w), a["ts"], a["tt"], 1.0, 1.0, p(loss), p(ds), p(row), a["M"], a["K"], None) == -1
    assert L.dinox_ibot_ce(p(s), p(t), p(c), p(w), 0.1, 0.04, 1.0, 1.0, p(loss), p(s), p(row), M, K, None) == -1
    assert L.dinox_ibot_put_mask(p(ds), p(c), p(w), 1, 4, 8, 5, None) == -1 and L.dinox_gather_rows(p(s), p(w), p(ds), 1, 4, 0, 0, 0, None) == -1
    torch.cuda.synchronize()
    assert bool((loss == 9.0).all()) and bool((ds == 9.0).all()) and bool((row == 9.0).all())


@pytest.mark.parametrize("K", [8, 1029])
def test_center_ema_from_sums_and_count(dx, K):
    """center = center mom + (sum / count) (1 - mom) against float64: a division, two products and an add, (4 + 2) u on the absolute
    terms; a count below 1 leaves the centre bit for bit what it was."""
    ops, _ = dx
    r = np.random.default_rng(K)
    c0, sums = r.standard_normal(K).astype(np.float32), (37 * r.standard_normal(K)).astype(np.float32)
    for count in (37.0, 1.0):
        sc = torch.from_numpy(np.concatenate([sums, [count]]).astype(np.float32)).to(DEV)
        c = torch.from_numpy(c0).to(DEV)
        ops.ibot_center_ema_(c, sc, 0.9)
        mom = np.float64(np.float32(0.9))
        mean = sums.astype(np.float64) / count
        want = c0 * mom + mean * (1.0 - mom)
        within(f"center_ema[{K},{count}]", c.cpu().numpy(), want, (4 + 2) * IO.U * (np.abs(c0 * mom) + np.abs(mean * (1.0 - mom))) + IO.TINY)
    for count in (0.0, 0.5, -3.0):
        sc = torch.from_numpy(np.concatenate([sums, [count]]).astype(np.float32)).to(DEV)
        c = torch.from_numpy(c0).to(DEV)
        ops.ibot_center_ema_(c, sc, 0.9)
        assert np.array_equal(c.cpu().numpy(), c0), count


# ------------------------------------------------------------------------------------------ engine
KW = dict(img_size=56, patch=14, dim=64, depth=2, heads=2, num_registers=4, scale_aware=True)      # the tiny ViT of tests/test_gpu_parity.py
OUT = 128


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().cpu().reshape(-1), torch.as_tensor(b).double().cpu().reshape(-1)
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def tiny_setup(seed=8, B=4):
    from oracle import dinox_oracle as O
    cfg = O.VitCfg(out_dim=OUT, **KW)
    g = torch.Generator().manual_seed(seed)
    sd = O.random_params(cfg, seed=seed)
    sd["backbone.mask_token"] = 0.3 * torch.randn(1, 1, KW["dim"], generator=g)
    tsd = {k: v + 0.01 * torch.randn(v.shape, generator=g) for k, v in sd.items()}
    batch = torch.randn(2 * B, 3, 56, 56, generator=g)
    sp = torch.rand(B, 3, generator=g) + 0.5
    locs = torch.randn(3 * B, 3, 28, 28, generator=g)
    return O, cfg, sd, tsd, batch, torch.cat([sp, sp], 0), locs, torch.cat([sp] * 3, 0)


def build_engine(arch, sd, tsd, hp, **kw):
    from dinox.engine import TrainEngine
    nets = [arch.DinoStudentTeacher(arch.PatchViT(mask_token="backbone.mask_token" in sd, **KW), OUT) for _ in range(2)]
    nets[0].load_state_dict(sd)
    nets[1].load_state_dict(tsd)
    return TrainEngine(nets[0].to(DEV), nets[1].to(DEV), OUT, hp, **kw), nets[0]


def tiny_mask(V=8, P=16, R=4, seed=0):
    from dinox.ibot import MaskGenerator
    m = MaskGenerator(seed, 4, registers=R, mask_prob=0.6).draw(V)
    assert 0 < len(np.unique(m.idx // P)) < V                        # some views masked, some not
    return m


@pytest.mark.parametrize("centering", ["ema", "sinkhorn"])
@pytest.mark.parametrize("crops", [False, True], ids=["global", "multicrop"])
def test_step_matches_the_plain_torch_objective(dx, crops, centering):
    """One fp32 step with ibot_weight > 0 against autograd on the same weights and masks: the loss, its terms, the grad-norm and the
    gradient of every parameter, mask_token among them (tolerances of test_step_multicrop_matches_oracle)."""
    ops, arch = dx
    from dinox.engine import StepHyperParams
    O, cfg, sd, tsd, batch, sp2, locs, spl = tiny_setup()
    mask = tiny_mask()
    hp = StepHyperParams(lr=1e-3, warmup_steps=1, max_steps=10, ema=0.99, ibot_weight=0.7, centering=centering)
    g = torch.Generator().manual_seed(1)
    center, pcenter = 0.1 * torch.randn(1, OUT, generator=g), 0.1 * torch.randn(1, OUT, generator=g)
    lo = dict(locs=locs, spl=spl) if crops else {}
    want, grads, t_p = IO.objective(O, cfg, sd, tsd, center, pcenter, batch, sp2, mask, O.HyperParams(lr=1e-3, warmup_steps=1, max_steps=10, ema=0.99),
                                    0.7, centering=centering, **lo)
    eng, student = build_engine(arch, sd, tsd, hp)
    eng.center.copy_(center)
    eng.ibot_center.copy_(pcenter)
    if crops:
        eng.step(batch.to(DEV), sp2.to(DEV), local_batch=locs.to(DEV), local_spacing=spl.to(DEV), patch_mask=mask.to(DEV))
    else:
        eng.step(batch.to(DEV), sp2.to(DEV), patch_mask=mask.to(DEV))
    got = eng.scalars()
    print({k: (got[k], want[k]) for k in want})
    for k in ("loss", "dino", "gram", "ibot", "grad_norm"):
        assert got[k] == pytest.approx(want[k], rel=1e-3), (k, got[k], want[k])
    names = [n for n, _ in student.named_parameters()]
    assert "backbone.mask_token" in names and float(grads["backbone.mask_token"].abs().max()) > 1e-6
    for n, p in zip(names, eng.params):
        if float(grads[n].abs().max()) > 1e-6:
            assert rel_l2(p.grad, grads[n]) < 2e-3, n
    # the patch centre moved towards the mean masked teacher row, after the loss used the old one
    moved = 0.9 * pcenter + 0.1 * t_p.mean(0, keepdim=True)
    assert rel_l2(eng.ibot_center, moved) < 1e-4


@pytest.mark.parametrize("crops", [False, True], ids=["global", "multicrop"])
def test_bf16_step_stays_close_to_the_fp32_step(dx, crops):
    """The throughput mode (--amp): bf16 patch rows take the mask token, the heads' operands are gathered in bf16 and the head's bf16
    input gradient is scattered back.  Against the fp32 step on the same weights and masks: every value finite, the loss and the term
    within 5 % (the distance smoke() allows the bf16 step), the gradient of every parameter -- mask_token among them -- within 10 % in
    relative L2 where it is not ~0 (bf16 carries 8 bits; the products of two blocks and a head compound a few of its 2^-9 roundings)."""
    ops, arch = dx
    from dinox.engine import StepHyperParams
    O, cfg, sd, tsd, batch, sp2, locs, spl = tiny_setup()
    mask = tiny_mask()
    hp = StepHyperParams(lr=1e-3, warmup_steps=1, max_steps=10, ema=0.99, ibot_weight=1.0)
    kw = dict(local_batch=locs.to(DEV), local_spacing=spl.to(DEV)) if crops else {}
    out = {}
    for dt in (None, torch.bfloat16):
        eng, student = build_engine(arch, sd, tsd, hp, amp_dtype=dt)
        eng.step(batch.to(DEV), sp2.to(DEV), patch_mask=mask.to(DEV), **kw)
        out[dt] = (eng.scalars(), {n: p.grad.clone() for (n, _), p in zip(student.named_parameters(), eng.params)}, eng.ibot_center.clone())
    (a, ga, ca), (b, gb, cb) = out[None], out[torch.bfloat16]
    assert all(np.isfinite(v) for v in b.values()) and all(bool(torch.isfinite(g).all()) for g in gb.values())
    for k in ("loss", "ibot", "dino"):
        assert b[k] == pytest.approx(a[k], rel=5e-2), (k, a[k], b[k])
    assert float(gb["backbone.mask_token"].abs().max()) > 0
    for n in ga:
        if float(ga[n].abs().max()) > 1e-6:
            assert rel_l2(gb[n], ga[n]) < 0.1, (n, rel_l2(gb[n], ga[n]))
    assert rel_l2(cb, ca) < 2e-2


def test_empty_mask_is_the_step_without_the_term(dx):
    """ibot_weight > 0 with nothing masked: the loss and every parameter after the update equal the ibot_weight = 0 step bit for bit, the
    term is reported as 0, mask_token receives a zero gradient and the patch centre does not move."""
    ops, arch = dx
    from dinox.engine import StepHyperParams
    from dinox.ibot import MaskGenerator
    O, cfg, sd, tsd, batch, sp2, locs, spl = tiny_setup()
    runs = []
    for weight in (0.0, 1.0):
        eng, _ = build_engine(arch, sd, tsd, StepHyperParams(lr=1e-3, warmup_steps=1, max_steps=10, ema=0.99, ibot_weight=weight, koleo_weight=0.1))
        kw = dict(patch_mask=MaskGenerator(0, 4, mask_prob=0.0).draw(8).to(DEV)) if weight else {}
        for _ in range(2):
            eng.step(batch.to(DEV), sp2.to(DEV), **kw)
        runs.append((eng.scalars(), eng.flat_p.clone(), eng.flat_t.clone(), eng.center.clone(), eng))
    (a, pa, ta, ca, _), (b, pb, tb, cb, eng) = runs
    assert "ibot" not in a and b["ibot"] == 0.0
    assert a["loss"] == b["loss"] and a["grad_norm"] == b["grad_norm"]
    assert torch.equal(pa, pb) and torch.equal(ta, tb) and torch.equal(ca, cb)
    assert not bool(eng.student.backbone.mask_token.grad.any()) and not bool(eng.ibot_center.any())      # a zero gradient; weight decay alone moves it


def test_three_steps_are_bit_reproducible(dx):
    ops, arch = dx
    from dinox.engine import StepHyperParams
    from dinox.ibot import MaskGenerator
    O, cfg, sd, tsd, batch, sp2, locs, spl = tiny_setup()
    outs = []
    for _ in range(2):
        eng, _ = build_engine(arch, sd, tsd, StepHyperParams(lr=1e-3, warmup_steps=1, max_steps=10, ema=0.99, ibot_weight=1.0))
        gen = MaskGenerator(4, 4, registers=4, mask_prob=0.8)
        losses = []
        for _ in range(3):
            eng.step(batch.to(DEV), sp2.to(DEV), patch_mask=gen.draw(8).to(DEV))
            losses.append((float(eng.last["loss"]), float(eng.last["ibot"])))
        outs.append((losses, eng.flat_p.clone(), eng.flat_t.clone(), eng.ibot_center.clone()))
    assert outs[0][0] == outs[1][0] and all(l[1] > 0 for l in outs[0][0])
    assert all(torch.equal(x, y) for x, y in zip(outs[0][1:], outs[1][1:]))


def test_accumulation_over_two_half_batches_matches_one_step(dx):
    """accumulation_steps = 2 over the two halves of a batch against one step on the whole batch (frozen centres, Gram off: the Gram
    term is a mean over samples too, but its normalisation is per batch); tolerances of test_gradient_accumulation_semantics."""
    ops, arch = dx
    from dinox.engine import StepHyperParams
    from dinox.ibot import make_mask
    O, cfg, sd, tsd, batch, sp2, locs, spl = tiny_setup(B=4)
    P, R, B = 16, 4, 4
    mask = tiny_mask()
    common = dict(ema=0.9, center_momentum=1.0, ibot_weight=1.0, gram_weight=0.0)
    e1, _ = build_engine(arch, sd, tsd, StepHyperParams(lr=1e-3 * 2 / 4, warmup_steps=0, max_steps=None, **common))
    e1.step(batch.to(DEV), sp2.to(DEV), patch_mask=mask.to(DEV))
    e2, _ = build_engine(arch, sd, tsd, StepHyperParams(lr=1e-3, warmup_steps=4, max_steps=20, **common), accumulation_steps=2)
    halves = []
    for h in range(2):                                      # samples 2h, 2h + 1: their view-1 and view-2 rows
        views = np.array([2 * h, 2 * h + 1, B + 2 * h, B + 2 * h + 1])
        where = {int(v): j for j, v in enumerate(views)}
        mine = [where[int(f // P)] * P + int(f % P) for f in mask.idx if int(f // P) in where]
        halves.append((batch[views].to(DEV), sp2[views].to(DEV), make_mask(mine, 4, P, R).to(DEV)))
    losses = []
    for x, s, m in halves:
        e2.step(x, s, patch_mask=m)
        losses.append(float(e2.last["ibot"]))
    assert e2.opt_steps == 1
    assert 0.5 * sum(losses) == pytest.approx(float(e1.last["ibot"]), rel=1e-5)
    d = (e2.flat_p - e1.flat_p).abs()
    assert float((d <= 1e-6 + 1e-4 * e1.flat_p.abs()).double().mean()) > 0.995 and float(d.max()) <= 1.1e-3


# ------------------------------------------------------------------------------------------ data parallel
def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


WORKER = os.path.join(ROOT, "tests", "_ibot_dp_worker.py")


def _single(tmp_path, name, **extra):
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_port()), **extra)
    env.pop("DINOX_DIST_BACKEND", None)
    out = str(tmp_path / name)
    r = subprocess.run([sys.executable, WORKER, out], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-2000:]
    return torch.load(out)


@pytest.mark.parametrize("centering", ["ema", "sinkhorn"])
def test_world_of_one_with_forced_collectives_changes_no_bit(tmp_path, centering):
    a = _single(tmp_path, "plain.pt", DINOX_TEST_CENTERING=centering)
    b = _single(tmp_path, "forced.pt", DINOX_TEST_CENTERING=centering, DINOX_DP_FORCE_COLLECTIVES="1")
    assert a["rows"] == b["rows"] == 27 and a["ibot"] > 0
    assert a["loss"] == b["loss"] and a["ibot"] == b["ibot"] and a["grad_norm"] == b["grad_norm"]
    for k in ("flat_p", "center", "ibot_center"):
        assert torch.equal(a[k], b[k]), k


def _two_ranks(tmp_path, backend, centering, idle=False):
    """``idle``: on the second step rank 1 holds no masked row (18 and 0 rows) and must still join every collective."""
    outs = [str(tmp_path / f"r{r}.pt") for r in range(2)]
    extra = dict(DINOX_TEST_CENTERING=centering, DINOX_TEST_IDLE="1" if idle else "")
    env = dict(os.environ, DINOX_DIST_BACKEND=backend, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_port()), WORLD_SIZE="2", DINOX_DIST_TIMEOUT_S="60",
               **extra)
    procs = [subprocess.Popen([sys.executable, WORKER, outs[r]], env=dict(env, RANK=str(r), LOCAL_RANK=str(r if backend == "nccl" else 0)),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(2)]
    logs = [p.communicate(timeout=240)[0].decode(errors="replace")[-1500:] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)
    a, b, ref = torch.load(outs[0]), torch.load(outs[1]), _single(tmp_path, "single.pt", **extra)
    assert (a["rows"], b["rows"], ref["rows"]) == (18, 9, 27)                                    # the ranks hold different numbers of rows
    assert (a["rows_last"], b["rows_last"], ref["rows_last"]) == ((18, 0, 18) if idle else (18, 9, 27))
    assert a["fired_in_backward"] == b["fired_in_backward"] >= a["buckets"] - 1                  # the idle rank exchanged no bucket from finish()
    for k in ("flat_p", "center", "ibot_center"):
        assert torch.equal(a[k], b[k]), k                                                        # ranks stay in lock-step
    assert 0.5 * (a["loss"] + b["loss"]) == pytest.approx(ref["loss"], rel=2e-4)
    assert 0.5 * (a["ibot"] + b["ibot"]) == pytest.approx(ref["ibot"], rel=2e-4)
    assert a["grad_norm"] == pytest.approx(ref["grad_norm"], rel=2e-3)
    for k in ("center", "ibot_center"):
        err, scale = float((a[k] - ref[k]).abs().max()), float(ref[k].abs().max())
        assert err <= 1e-7 + 1e-4 * scale, (k, err, scale)
    d = (a["flat_p"] - ref["flat_p"]).abs()
    assert float((d <= 1e-5 + 1e-4 * ref["flat_p"].abs()).double().mean()) > 0.995 and float(d.max()) <= 2.5e-3


def test_two_ranks_on_one_gpu_match_the_single_rank_step(tmp_path):
    """Two gloo ranks on this GPU (as test_engine_data_parallel_two_ranks_match_single_process) with 18 and 9 masked rows against
    the single-rank step over the whole batch, at that test's tolerances.  EMA centring: the all-gathers of ops.sk_center's
    data-parallel path take the [world, K] <- [K] form that RCCL accepts and gloo refuses, so Sinkhorn over ranks runs below only."""
    _two_ranks(tmp_path, "gloo", "ema")


def test_a_rank_without_masked_rows_joins_every_collective(tmp_path):
    """As above, but on the second step rank 1 masks nothing: it adds zeros to the patch centre's sums, announces mask_token's zero
    gradient so that its bucket is exchanged after backward on both ranks alike, and the result is still the single-rank step's."""
    _two_ranks(tmp_path, "gloo", "ema", idle=True)


@pytest.mark.parametrize("centering,idle", [("ema", False), ("sinkhorn", False), ("sinkhorn", True)])
def test_two_gpus_match_the_single_rank_step(tmp_path, centering, idle):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    _two_ranks(tmp_path, "nccl", centering, idle)


# ------------------------------------------------------------------------------------------ command line
COMMON = ["--config", "custom", "--vit-patch", "8", "--vit-dim", "32", "--vit-depth", "2", "--vit-heads", "2", "--out-dim", "64", "--img-size", "32",
          "--batch-size", "8", "--synthetic", "32", "--num-workers", "0", "--warmup-steps", "2", "--lr", "1e-3", "--ckpt-every", "4", "--scale-aware",
          "--ibot-weight", "1.0", "--ibot-mask-prob", "0.7"]


def test_cli_trains_logs_checkpoints_resumes_and_the_backbone_loads(dx, cli, tmp_path, capsys):
    """Eight steps with --ibot-weight 1: finite losses, `ibot` in the log line and in every JSON record, the checkpoint holds the patch
    centre and the mask token; --resume restores both and goes on; load_model + encode of the checkpoint equals the same weights without
    the key."""
    import zoo.encode as enc
    import zoo.hub as hub
    log1, log2 = tmp_path / "a.jsonl", tmp_path / "b.jsonl"
    cli.main(COMMON + ["--run-dir", str(tmp_path / "runs"), "--max-steps", "8", "--log-json", str(log1)])
    out = capsys.readouterr().out
    assert "ibot_weight=1.0" in out and " ibot=" in out and "final_checkpoint=" in out
    rec = [json.loads(l) for l in log1.read_text().splitlines()]
    assert [r["step"] for r in rec] == list(range(8)) and all(set(r) == {"step", "loss", "lr", "ibot"} for r in rec)
    assert all(np.isfinite(r["loss"]) and np.isfinite(r["ibot"]) for r in rec) and sum(r["ibot"] > 0 for r in rec) >= 6
    run = sorted((tmp_path / "runs").iterdir())[-1]
    ck = torch.load(run / "checkpoint_final_00000008.pth", map_location="cpu", weights_only=False)
    assert ck["ibot_center"].shape == (1, 64) and bool(ck["ibot_center"].any()) and ck["config"]["ibot_weight"] == 1.0
    assert bool(ck["student"]["backbone.mask_token"].any()) and "backbone.mask_token" in ck["teacher"]
    # --resume, through the script's own path.  The sampler of the dino data path starts its order again on a resume (what it always did:
    # step-keyed batches would move the view draws of the seed, which must stay what they are without the flag), so step 8 of a resumed
    # run sees other images than step 8 of an uninterrupted one and cannot equal it.  What the script restores is held to equality
    # instead: resumed at step 8 with --max-steps 8 it takes no step and writes what it restored -- weights and mask token of both nets,
    # Adam moments and step, both centres -- which must be the uninterrupted checkpoint bit for bit; and the mask of step 8 is the
    # function of (seed, rank, step) the uninterrupted run would have called.
    kept = tmp_path / "uninterrupted.pth"
    kept.write_bytes((run / "checkpoint_final_00000008.pth").read_bytes())
    cli.main(COMMON + ["--run-dir", str(tmp_path / "runs"), "--max-steps", "8", "--resume", "auto"])
    assert "resumed_from_step=8" in capsys.readouterr().out
    back = torch.load(run / "checkpoint_final_00000008.pth", map_location="cpu", weights_only=False)
    assert back["step"] == ck["step"] == 8
    for entry in ("student", "teacher"):
        assert list(back[entry]) == list(ck[entry]) and all(torch.equal(back[entry][k], ck[entry][k]) for k in ck[entry]), entry
    assert torch.equal(back["ibot_center"], ck["ibot_center"]) and torch.equal(back["dino_loss"]["center"], ck["dino_loss"]["center"])
    assert set(back["opt"]["state"]) == set(ck["opt"]["state"])
    for i, st in ck["opt"]["state"].items():
        assert all(torch.equal(torch.as_tensor(st[k]), torch.as_tensor(back["opt"]["state"][i][k])) for k in st), i
    args = cli.parse_cli(COMMON)
    m8, again, m7 = (cli.ibot_step_mask(args, 0, s_, 4, 4) for s_ in (8, 8, 7))
    assert m8.count > 0 and all(np.array_equal(x, y) for x, y in zip(m8.triple(), again.triple())) and not np.array_equal(m8.idx, m7.idx)
    # ... and it goes on from there: steps 8 and 9, logged with the term, inside the reference canary's continuity band
    cli.main(COMMON + ["--run-dir", str(tmp_path / "runs"), "--max-steps", "10", "--log-json", str(log2), "--resume", "auto"])
    assert "resumed_from_step=8" in capsys.readouterr().out
    cont = [json.loads(l) for l in log2.read_text().splitlines()]
    assert [r["step"] for r in cont] == [8, 9] and all(np.isfinite(r["loss"]) and "ibot" in r for r in cont)
    assert 0.25 < cont[0]["loss"] / rec[-1]["loss"] < 3.0
    path = kept
    bare = dict(ck, student={k: v for k, v in ck["student"].items() if k != "backbone.mask_token"})
    torch.save(bare, tmp_path / "bare.pth")
    over = {"patch": 8, "num_registers": 4}
    a, b = hub.load_model(str(path), device=DEV, config_override=over), hub.load_model(str(tmp_path / "bare.pth"), device=DEV, config_override=over)
    img = np.random.default_rng(0).normal(40, 200, size=(48, 48)).astype(np.float32)
    fa, fb = (enc.encode(m, img, pixel_spacing=(0.7, 0.7), slice_thickness=2.0) for m in (a, b))
    assert fa.shape == (1, 1, 32) and torch.isfinite(fa).all() and torch.equal(fa, fb)


def test_view_draws_and_initial_weights_do_not_move_with_the_flag(dx, cli, tmp_path, monkeypatch):
    """Two runs of the script from one --train-seed, without and with --ibot-weight: every batch and spacing handed to the engine and the
    weights the first step starts from are bit for bit the same (the mask token aside, which is new and zero)."""
    seen = {}
    real = cli.TrainEngine.step

    def spy(self, batch, spacing2b=None, *a, **kw):
        rec = seen[tag]
        if not rec:
            rec.append({k: v.detach().cpu().clone() for k, v in self.student.state_dict().items()})
        rec.append((batch.detach().cpu().clone(), spacing2b.detach().cpu().clone()))
        return real(self, batch, spacing2b, *a, **kw)
    monkeypatch.setattr(cli.TrainEngine, "step", spy)
    base = [a for a in COMMON if a not in ("--ibot-weight", "1.0", "--ibot-mask-prob", "0.7")]
    for tag, extra in (("off", []), ("on", ["--ibot-weight", "1.0", "--ibot-mask-prob", "0.7"])):
        seen[tag] = []
        cli.main(base + extra + ["--run-dir", str(tmp_path / tag), "--max-steps", "3"])
    off, on = seen["off"], seen["on"]
    assert len(off) == len(on) == 4
    assert set(on[0]) - set(off[0]) == {"backbone.mask_token"} and not bool(on[0]["backbone.mask_token"].any())
    assert all(torch.equal(off[0][k], on[0][k]) for k in off[0])
    for (xa, sa), (xb, sb) in zip(off[1:], on[1:]):
        assert torch.equal(xa, xb) and torch.equal(sa, sb)


def test_weight_zero_run_writes_the_keys_it_always_wrote(dx, cli, tmp_path, capsys):
    base = [a for a in COMMON if a not in ("--ibot-weight", "1.0", "--ibot-mask-prob", "0.7")]
    log = tmp_path / "z.jsonl"
    cli.main(base + ["--run-dir", str(tmp_path / "runs"), "--max-steps", "2", "--log-json", str(log)])
    assert " ibot=" not in capsys.readouterr().out
    assert all(set(json.loads(l)) == {"step", "loss", "lr"} for l in log.read_text().splitlines())
    run = sorted((tmp_path / "runs").iterdir())[-1]
    ck = torch.load(run / "checkpoint_final_00000002.pth", map_location="cpu", weights_only=False)
    assert set(ck) == {"step", "student", "teacher", "opt", "scaler", "dino_loss", "rng", "config"}
    assert "backbone.mask_token" not in ck["student"] and "ibot_weight" not in ck["config"]


def test_checkpoint_round_trip_gives_the_uninterrupted_next_step(dx, cli, tmp_path):
    """save_checkpoint / load_checkpoint of the training script around an engine: after the round trip into a FRESH engine the next step on
    the same batch and mask equals the uninterrupted engine's bit for bit (weights, Adam state, both centres, mask token)."""
    ops, arch = dx
    from dinox.engine import StepHyperParams
    from dinox.ibot import MaskGenerator
    O, cfg, sd, tsd, batch, sp2, locs, spl = tiny_setup()
    hp = StepHyperParams(lr=1e-3, warmup_steps=1, max_steps=10, ema=0.99, ibot_weight=1.0)
    masks = [MaskGenerator(s, 4, registers=4, mask_prob=0.8).draw(8).to(DEV) for s in range(3)]
    e1, s1 = build_engine(arch, sd, tsd, hp)
    for m in masks[:2]:
        e1.step(batch.to(DEV), sp2.to(DEV), patch_mask=m)
    conf = cli.TrainingConfig(model=cli.ModelConfig("custom", 14, 64, 2, 2), lr=1e-3, scale_aware=True)
    cli.save_checkpoint(tmp_path / "c.pth", 2, s1, e1.teacher, e1, conf)
    e2, s2 = build_engine(arch, {k: torch.zeros_like(v) for k, v in sd.items()}, {k: torch.zeros_like(v) for k, v in sd.items()}, hp)
    step, _ = cli.load_checkpoint(tmp_path / "c.pth", s2, e2.teacher, e2, DEV, scale_aware=True)
    assert step == 2 and torch.equal(e2.ibot_center, e1.ibot_center) and torch.equal(e2.flat_p, e1.flat_p)
    for e in (e1, e2):
        e.step(batch.to(DEV), sp2.to(DEV), patch_mask=masks[2])
    assert float(e1.last["loss"]) == float(e2.last["loss"]) and float(e1.last["ibot"]) == float(e2.last["ibot"]) > 0
    assert torch.equal(e1.flat_p, e2.flat_p) and torch.equal(e1.flat_t, e2.flat_t) and torch.equal(e1.ibot_center, e2.ibot_center)


def test_zz_report_error_to_bound_ratios():
    """Not a check of its own: prints the largest error / bound ratio every kernel test above saw (each was asserted <= 1 there)."""
    assert all(v <= 1.0 for v in RATIOS.values())
    print("error/bound", json.dumps({k: round(v, 4) for k, v in sorted(RATIOS.items())}))
