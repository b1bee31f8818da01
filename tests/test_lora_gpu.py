"""GPU tests of the LoRA path: csrc/lora.hip against the float64 oracle (tests/_lora_oracle.py) with a-priori elementwise bounds,
ops.LoraLinearFn, zoo.peft on a tiny ViT, and scripts/finetune_lora.py end to end.

dinox_lora_up and dinox_lora_merge take fp32 tensors only (u, res and W are fp32 in both modes by the adapter's precision rules), so the
operand mode (fp32 / bf16) parametrises down, grad, dropout and LoraLinearFn."""
import ctypes
import importlib.util
import json
import os
import sys

import numpy as np
import pytest
import torch

import _lora_oracle as LO
from conftest import ROOT
from oracle.gemm_bounds import CANARY_F32, U32

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MS = (1, 5, 130, 402)                  # 130: more than one 128-row chunk with a ragged tail
DIMS = (8, 36, 384, 1152)              # all multiples of 4: the scalar widths, ragged second tiles and misaligned operands are tests/test_lora_paths_gpu.py
RANKS = (1, 8, 16, 64)
MODES = ("fp32", "bf16")
RATIOS: dict = {}


def tdt(mode):
    return torch.bfloat16 if mode == "bf16" else torch.float32


def operand(rng, shape, mode, scale=1.0):
    """-> (device tensor in the mode's dtype, its exact values as float64)."""
    t = torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32)).to(tdt(mode))
    return t.to(DEV), t.double().numpy()


def f32(rng, shape, scale=1.0):
    a = (rng.standard_normal(shape) * scale).astype(np.float32)
    return torch.from_numpy(a).to(DEV), a.astype(np.float64)


def judge(name, got, ref, bound):
    got = got.detach().double().cpu().numpy().reshape(ref.shape)
    assert np.isfinite(got).all(), f"{name}: non-finite output"
    err = np.abs(got - ref)
    ratio = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    RATIOS[name] = max(RATIOS.get(name, 0.0), ratio)
    assert (err <= bound).all(), f"{name}: error / bound = {ratio:.3g} at {np.unravel_index((err / np.maximum(bound, 1e-300)).argmax(), err.shape)}"


# ------------------------------------------------------------------------------------------ kernels against the oracle
@pytest.mark.parametrize("r", RANKS)
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("mode", MODES)
def test_down(mode, M, r):
    from dinox import ops
    for K in DIMS:
        rng = np.random.default_rng([1, M, K, r])
        x, x64 = operand(rng, (M, K), mode)
        S, S64 = f32(rng, (r, K))
        ref, bound = LO.down(x64, S64)
        judge(f"down[{mode}]", ops.lora_down(x, S, 0), ref, bound)
        judge(f"down[{mode}]", ops.lora_down(x, S.t().contiguous(), 1), ref, bound)


@pytest.mark.parametrize("r", RANKS)
@pytest.mark.parametrize("M", MS)
def test_up(M, r):
    from dinox import ops
    for N in DIMS:
        rng = np.random.default_rng([2, M, N, r])
        u, u64 = f32(rng, (M, r))
        S, S64 = f32(rng, (N, r))
        res, res64 = f32(rng, (M, N))
        for with_res in (False, True):
            ref, bound = LO.up(u64, S64, 0.375, res64 if with_res else None)
            rt = res if with_res else None
            judge("up", ops.lora_up(u, S, 0.375, res=rt, layout=0), ref, bound)
            judge("up", ops.lora_up(u, S.t().contiguous(), 0.375, res=rt, layout=1), ref, bound)
        t = res.clone()                                                                    # res == t: in place
        judge("up", ops.lora_up(u, S, 0.375, res=t, layout=0, out=t), *LO.up(u64, S64, 0.375, res64))


@pytest.mark.parametrize("r", RANKS)
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("mode", MODES)
def test_grad(mode, M, r):
    from dinox import ops
    for K in DIMS:
        for N in DIMS:
            rng = np.random.default_rng([3, M, K, N, r])
            xl, xl64 = operand(rng, (M, K), mode)
            dy, dy64 = operand(rng, (M, N), mode)
            A, A64 = f32(rng, (r, K), 0.1)
            B, B64 = f32(rng, (N, r), 0.1)
            dA, dB = ops.lora_grad(xl, dy, A, B, 2.0)
            rA, eA, rB, eB = LO.grad(xl64, dy64, A64, B64, 2.0)
            judge(f"grad dA[{mode}]", dA, rA, eA)
            judge(f"grad dB[{mode}]", dB, rB, eB)


@pytest.mark.parametrize("r", RANKS)
def test_merge(r):
    from dinox import ops
    for N in DIMS:
        for K in DIMS:
            rng = np.random.default_rng([4, N, K, r])
            W, W64 = f32(rng, (N, K))
            A, A64 = f32(rng, (r, K), 0.1)
            B, B64 = f32(rng, (N, r), 0.1)
            for sign in (1, -1):
                judge("merge", ops.lora_merge(W, A, B, 2.0, sign), *LO.merge(W64, A64, B64, 2.0, sign))
            Wc = W.clone()
            judge("merge", ops.lora_merge(Wc, A, B, 2.0, 1, out=Wc), *LO.merge(W64, A64, B64, 2.0, 1))


# ------------------------------------------------------------------------------------------ dinox_lora_grad: bits and footprint
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("M,K,N,r", [(130, 36, 1152, 1), (402, 384, 36, 8), (130, 1152, 384, 64), (5, 8, 8, 16)])
def test_grad_is_reproducible_and_stays_in_its_buffers(mode, M, K, N, r):
    from dinox import _lib
    from dinox.ops import _code, _p, _stream
    rng = np.random.default_rng([5, M, K, N, r])
    xl, _ = operand(rng, (M, K), mode)
    dy, _ = operand(rng, (M, N), mode)
    A, _ = f32(rng, (r, K))
    B, _ = f32(rng, (N, r))
    G = 1024
    nws = _lib.lib.dinox_lora_grad_ws_bytes(M, K, N, r) // 4
    assert nws == -(-M // LO.CHUNK) * (r * K + N * r)
    canary = int(CANARY_F32)
    runs = []
    for _ in range(2):
        bufs = [torch.full((n + 2 * G,), canary, dtype=torch.int32, device=DEV) for n in (r * K, N * r, nws)]
        ptrs = [b.data_ptr() + 4 * G for b in bufs]
        _lib.check(_lib.lib.dinox_lora_grad(_p(xl), _p(dy), _p(A), _p(B), 1.5, ptrs[0], ptrs[1], ptrs[2], M, K, N, r, _code(xl.dtype), _stream()),
                   "dinox_lora_grad")
        torch.cuda.synchronize()
        for b in bufs:
            assert (b[:G] == canary).all() and (b[-G:] == canary).all(), "written outside the buffer"
        assert not (bufs[0][G:-G] == canary).any() and not (bufs[1][G:-G] == canary).any(), "an output element was left unwritten"
        runs.append((bufs[0][G:-G].clone(), bufs[1][G:-G].clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


# ------------------------------------------------------------------------------------------ dropout
@pytest.mark.parametrize("p", (0.0, 0.05, 0.5))
@pytest.mark.parametrize("n", (1, 7, 4099))
@pytest.mark.parametrize("mode", MODES)
def test_dropout_mask_is_the_oracles(mode, n, p):
    from dinox import ops
    for offset in (0, (1 << 33) + 5):
        seed = 0x123456789ABCDEF
        keep = LO.keep_mask(n, p, seed, offset)
        ones = torch.ones(n, dtype=tdt(mode), device=DEV)
        got = ops.lora_dropout(ones, p, seed, offset)
        assert np.array_equal(got.float().cpu().numpy() != 0.0, keep), (n, p, offset)
        rng = np.random.default_rng([6, n])
        x, x64 = operand(rng, (n,), mode)
        ref, e = LO.dropout(x64, p, seed, offset, mode == "bf16")
        judge(f"dropout[{mode}]", ops.lora_dropout(x, p, seed, offset), ref, e)
        y = x.clone()
        ops.lora_dropout(y, p, seed, offset, out=y)                                         # in place
        assert torch.equal(y, ops.lora_dropout(x, p, seed, offset))
        big = torch.ones(n + 1, dtype=tdt(mode), device=DEV)                                # a view that is not 16-byte aligned
        assert np.array_equal(ops.lora_dropout(big[1:], p, seed, offset).float().cpu().numpy() != 0.0, keep)


# ------------------------------------------------------------------------------------------ LoraLinearFn
FN_SHAPES = [((5,), 36, 20, 4), ((2, 65), 384, 96, 8)]          # leading dims of x, K, N, r


def _layer(rng, lead, K, N, r, mode, zero_B=False):
    from dinox import ops  # noqa: F401
    x = torch.from_numpy(rng.standard_normal((*lead, K)).astype(np.float32)).to(DEV)
    W, _ = f32(rng, (N, K), K ** -0.5)
    b, _ = f32(rng, (N,), 0.1)
    A, _ = f32(rng, (r, K), K ** -0.5)
    B, _ = f32(rng, (N, r), 0.0 if zero_B else 0.3)
    res, _ = f32(rng, (*lead, N))
    dy = torch.from_numpy(rng.standard_normal((*lead, N)).astype(np.float32)).to(DEV)
    return x, W, b, A, B, res, dy


def _vals(t, mode):
    """The values the kernels see: the tensor rounded to the mode's operand dtype, as float64 rows."""
    return t.detach().to(tdt(mode)).double().cpu().numpy().reshape(-1, t.shape[-1])


@pytest.mark.parametrize("with_res", (False, True))
@pytest.mark.parametrize("lead,K,N,r", FN_SHAPES)
@pytest.mark.parametrize("mode", MODES)
def test_fn_with_zero_B_is_linear_fn(mode, lead, K, N, r, with_res):
    from dinox import ops
    x, W, b, A, B, res, dy = _layer(np.random.default_rng([7, K, N]), lead, K, N, r, mode, zero_B=True)
    with ops.compute_dtype(tdt(mode)):
        want = ops.LinearFn.apply(x, W, b, res if with_res else None, None)
        got = ops.lora_linear(x, W, b, A, B, 2.0, 0.0, None, res if with_res else None)
        none = ops.lora_linear(x, W, b, None, None, 2.0, 0.0, None, res if with_res else None)
    assert got.dtype == want.dtype and torch.equal(got, want)
    assert torch.equal(none, want)


@pytest.mark.parametrize("p", (0.0, 0.5))
@pytest.mark.parametrize("with_res", (False, True))
@pytest.mark.parametrize("lead,K,N,r", FN_SHAPES)
@pytest.mark.parametrize("mode", MODES)
def test_fn_forward_and_gradients(mode, lead, K, N, r, with_res, p):
    from dinox import ops
    x, W, b, A, B, res, dy = _layer(np.random.default_rng([8, K, N]), lead, K, N, r, mode)
    x.requires_grad_(True)
    A.requires_grad_(True)
    B.requires_grad_(True)
    s, seed, offset = 2.0, 77, 3
    bf = mode == "bf16"
    with ops.compute_dtype(tdt(mode)):
        y = ops.lora_linear(x, W, b, A, B, s, p, (seed, offset), res if with_res else None)
        y.backward(dy.to(y.dtype))
    assert W.grad is None and b.grad is None                                                # a frozen base gets no gradient
    assert y.dtype == (torch.float32 if (with_res or not bf) else torch.bfloat16)
    x64, W64, dy64 = _vals(x, mode), _vals(W, mode), _vals(dy, mode)
    A64, B64, b64 = A.detach().double().cpu().numpy(), B.detach().double().cpu().numpy(), b.double().cpu().numpy()
    res64 = res.double().cpu().numpy().reshape(-1, N) if with_res else None
    ref, e, xl64, e_xl = LO.lora_linear(x64, W64, b64, A64, B64, s, res64, p, seed, offset, bf16_ops=bf, bf16_out=y.dtype == torch.bfloat16)
    tag = f"[{mode}{', p' if p else ''}]"
    judge("fn y" + tag, y, ref, e)
    back = LO.lora_linear_bwd(x64, xl64, e_xl, dy64, W64, A64, B64, s, p, seed, offset, bf16_out=bf)
    judge("fn dx" + tag, x.grad, *back["dx"])
    judge("fn dA" + tag, A.grad, *back["dA"])
    judge("fn dB" + tag, B.grad, *back["dB"])


@pytest.mark.parametrize("lead,K,N,r", FN_SHAPES)
@pytest.mark.parametrize("mode", MODES)
def test_fn_base_gradients(mode, lead, K, N, r):
    """Frozen base: no dW product, grad None.  Trainable base: dW and db are LinearFn's, bit for bit (the same weight_grad call)."""
    from dinox import ops
    x, W, b, A, B, res, dy = _layer(np.random.default_rng([9, K, N]), lead, K, N, r, mode)
    traced = []
    with ops.compute_dtype(tdt(mode)):
        A.requires_grad_(True)
        y = ops.lora_linear(x, W, b, A, B, 2.0, 0.0, None, res)
        ops.TRACE_KERNELS = traced
        try:
            y.backward(dy)
        finally:
            ops.TRACE_KERNELS = None
        assert W.grad is None and b.grad is None and traced == [], traced                   # x needs no gradient either: no product at all
        W.requires_grad_(True)
        b.requires_grad_(True)
        ops.lora_linear(x, W, b, A, B, 2.0, 0.0, None, res).backward(dy)
        dW, db = W.grad.clone(), b.grad.clone()
        W.grad = b.grad = None
        ops.LinearFn.apply(x, W, b, res, None).backward(dy)
    assert torch.equal(dW, W.grad) and torch.equal(db, b.grad)


def test_bf16_adapter_below_half_an_ulp_of_W_is_visible():
    """||s B A|| = 2^-12 ||W||: folded into a bf16 weight the adapter vanishes (shown on the host below); as the fp32 addend of the product it
    moves the bf16-mode output by the oracle's delta."""
    from dinox import ops
    M, K, N, r, s = 130, 384, 96, 8, 2.0
    rng = np.random.default_rng(10)
    x, W, b, A, B, _, _ = _layer(rng, (M,), K, N, r, "bf16")
    B *= float(2.0 ** -12 * W.norm() / (s * (B @ A).norm()))
    folded = (W + s * B @ A).bfloat16()
    assert (folded == W.bfloat16()).float().mean().item() > 0.8                            # what training through a merged bf16 weight would see
    zero = torch.zeros((M, N), dtype=torch.float32, device=DEV)
    with ops.compute_dtype(torch.bfloat16):
        # both go through the SAME dinox_gemm configuration (shape, RESIDUAL epilogue, fp32 output), which is reproducible to the bit, so
        # the two outputs hold the same accumulator g: base = fl(g + 0), got = fl(g + t)
        base = ops.LinearFn.apply(x, W, b, zero, None)
        got = ops.lora_linear(x, W, b, A, B, s, 0.0, None, zero)
    x64, W64 = _vals(x, "bf16"), _vals(W, "bf16")
    A64, B64 = A.double().cpu().numpy(), B.double().cpu().numpy()
    u, e_u = LO.down(x64, A64)
    delta, e_t = LO.up(u, B64, s, e_u=e_u)
    v, e_v = LO.base_product(x64, W64, b.double().cpu().numpy())
    bound = e_t + 3 * U32 * (np.abs(v) + e_v + np.abs(delta))          # t's own error, the add g + t, the subtraction
    assert np.median(np.abs(delta)) > 8 * np.median(bound), "the case has no power: the bound swallows the adapter's term"
    judge("bf16 visibility", got - base, delta, bound)


# ------------------------------------------------------------------------------------------ zoo.peft on a tiny ViT
TINY = dict(img_size=32, patch=8, dim=32, depth=2, heads=2, scale_aware=True)


def _tiny(seed=0):
    import zoo.arch as arch
    torch.manual_seed(seed)
    m = arch.PatchViT(**TINY)
    with torch.no_grad():                                   # a fresh scale embedding is a no-op: make spacing matter
        m.scale_embed.mlp[2].weight.normal_(0, 0.05)
    return m.to(DEV).eval()


def _inputs():
    g = torch.Generator().manual_seed(11)
    return torch.randn(3, 3, 32, 32, generator=g).to(DEV), (torch.rand(3, 3, generator=g) + 0.5).to(DEV)


class _OtherLinear(torch.nn.Module):
    """Wraps a Linear so that the block is no longer fusable: the plain model then runs its per-op path (LinearFn, GeluFn)."""
    takes_residual = True

    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def forward(self, x, residual=None, out_dtype=None):
        return self.inner(x, residual=residual, out_dtype=out_dtype)


@pytest.mark.parametrize("mode", MODES)
def test_model_wrapped_forward_equals_the_per_op_path_while_B_is_zero(mode):
    from dinox import ops
    from zoo.peft import apply_lora
    x, sp = _inputs()
    plain = _tiny()
    for blk in plain.blocks:
        for parent, name in ((blk.attn, "qkv"), (blk.attn, "proj"), (blk.mlp, "fc1"), (blk.mlp, "fc2")):
            setattr(parent, name, _OtherLinear(getattr(parent, name)))
    wrapped = apply_lora(_tiny(), rank=4).eval()
    assert not any(b._fusable() for b in wrapped.base_model.model.blocks)
    with torch.no_grad(), ops.compute_dtype(tdt(mode)):
        want = plain(x, spacing=sp)
        got = wrapped(x, spacing=sp)
        fused = _tiny()(x, spacing=sp)
    assert got.shape == fused.shape == (3, 1 + 16 + 4, 32) and got.dtype == torch.float32
    assert torch.equal(got, want)


def test_model_one_step_moves_adapter_and_head_only():
    ft = _script()
    from zoo.peft import apply_lora
    x, sp = _inputs()
    model = ft.FinetuneModel(apply_lora(_tiny(), rank=4, dropout=0.0), 32, 2).to(DEV)
    opt = ft.ArenaAdamW([([p for p in model.parameters() if p.requires_grad], 1e-2)], 0.0)
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model.train()
    for _ in range(2):                                       # B starts at zero: A's gradient is zero until B has moved once
        opt.zero_grad()
        ft.task_loss(model(x, spacing=sp), torch.tensor([0, 1, 0], device=DEV), "classification").backward()
        opt.step(1.0)
    moved = {k for k, v in model.state_dict().items() if not torch.equal(v, before[k])}
    expect = {k for k in before if ".lora_" in k or k.startswith("head.")}
    assert moved == expect, (sorted(moved - expect)[:4], sorted(expect - moved)[:4])


def _random_adapter(wrapped, seed=5):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, p in wrapped.named_parameters():
            if ".lora_B." in k:
                p.copy_(torch.randn(p.shape, generator=g).to(DEV) * 0.05)


def test_model_merge_unmerge_and_unload():
    from dinox import ops
    from zoo.peft import apply_lora
    x, sp = _inputs()
    wrapped = apply_lora(_tiny(), rank=4).eval()
    _random_adapter(wrapped)
    vit = wrapped.base_model.model
    w0 = {k: v.detach().clone() for k, v in vit.state_dict().items() if k.endswith("base_layer.weight")}
    layers = {k[:-len(".base_layer.weight")]: vit.get_submodule(k[:-len(".base_layer.weight")]) for k in w0}
    with torch.no_grad(), ops.compute_dtype(torch.float32):
        want = wrapped(x, spacing=sp)
        wrapped.merge_adapter()
        merged = wrapped(x, spacing=sp)
        wrapped.unmerge_adapter()
        for k, w in w0.items():                              # W + d - d: one add and one subtract of d = s B A, each rounded once
            m = layers[k[:-len(".base_layer.weight")]]
            d = (m.scaling * m.lora_B["default"].weight.double() @ m.lora_A["default"].weight.double()).abs()
            bound = 2 * float(U32) * (w.double().abs() + 2 * d) + 2 * LO.gam(m.r + 2) * d
            assert ((vit.state_dict()[k].double() - w.double()).abs() <= bound).all(), k
        again = wrapped(x, spacing=sp)
        plain = wrapped.merge_and_unload()
        unloaded = plain(x, spacing=sp)
    import zoo.arch as arch
    assert type(plain) is arch.PatchViT and all(b._fusable() for b in plain.blocks)
    # fp32 bound of the comparison, to first order: the two sides are fp32 forward passes of the same function whose 8 adapted products
    # (4 per block) each sum K + r <= 128 + 4 terms in another order or with s B A rounded into W first: gamma_(K + r + 2) relative per
    # product, added over the 8 products, on outputs of magnitude max |want| (the final LayerNorm fixes their scale)
    tol = 8 * LO.gam(128 + 4 + 2) * want.abs().max().item()
    for name, t in (("merged", merged), ("unloaded", unloaded), ("unmerged", again)):
        err = (t - want).abs().max().item()
        RATIOS[f"model {name} vs wrapped"] = err / tol
        assert err <= tol, (name, err)


# ------------------------------------------------------------------------------------------ scripts/finetune_lora.py
def _script():
    if "finetune_lora" in sys.modules:
        return sys.modules["finetune_lora"]
    spec = importlib.util.spec_from_file_location("finetune_lora", os.path.join(ROOT, "dino-x_amd", "scripts", "finetune_lora.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def backbone_dir(tmp_path_factory):
    from zoo.hub import export_hub_checkpoint
    d = tmp_path_factory.mktemp("tiny_hub")
    export_hub_checkpoint(_tiny(), d, config=dict(TINY, mlp_ratio=4.0, num_registers=4))
    return d


def _run(ft, backbone_dir, out, *extra):
    argv = ["--backbone", str(backbone_dir), "--synthetic", "64", "--epochs", "3", "--batch-size", "16", "--rank", "4", "--seed", "0",
            "--output", str(out), *extra]
    return ft.run(ft.build_parser().parse_args(argv))


@pytest.fixture(scope="module")
def first_run(backbone_dir, tmp_path_factory):
    out = tmp_path_factory.mktemp("adapter_a")
    return out, _run(_script(), backbone_dir, out)


def test_script_trains_and_writes_its_files(first_run):
    out, res = first_run
    hist = res["config"].train_loss_history
    print("train loss per epoch:", hist)
    assert len(hist) == 3 and hist[-1] < hist[0]
    assert {"adapter_config.json", "adapter_model.safetensors", "head.pth", "finetune_config.json"} == {p.name for p in out.iterdir()}
    cfg = json.loads((out / "finetune_config.json").read_text())
    assert cfg["rank"] == 4 and cfg["train_samples"] == 48 and cfg["val_samples"] == 16


def test_script_reload_reproduces_validation_logits(first_run, backbone_dir):
    ft = _script()
    from zoo.hub import load_model
    from zoo.peft import load_adapter
    out, res = first_run
    model = ft.FinetuneModel(load_adapter(load_model(str(backbone_dir), device=DEV), out), 32, 2).to(DEV)
    model.head.load_state_dict(torch.load(out / "head.pth", map_location=DEV, weights_only=True))
    loader = torch.utils.data.DataLoader(res["val_dataset"], batch_size=16, shuffle=False)
    _, _, logits = ft.validate(model, loader, torch.device(DEV), "classification", 2, True, True)
    assert torch.equal(logits, res["val_logits"])


def test_script_same_seed_same_adapter(first_run, backbone_dir, tmp_path):
    from safetensors.torch import load_file
    out, _ = first_run
    _run(_script(), backbone_dir, tmp_path)
    a, b = load_file(str(out / "adapter_model.safetensors")), load_file(str(tmp_path / "adapter_model.safetensors"))
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    assert torch.equal(torch.load(out / "head.pth", weights_only=True)["weight"], torch.load(tmp_path / "head.pth", weights_only=True)["weight"])


def test_script_unfreeze_blocks_writes_that_blocks_weights(backbone_dir, tmp_path):
    _run(_script(), backbone_dir, tmp_path, "--unfreeze-blocks", "1")
    state = torch.load(tmp_path / "unfrozen_blocks.pth", weights_only=True)
    import zoo.arch as arch
    names = {f"blocks.1.{n}".replace(".qkv.", ".qkv.base_layer.").replace(".proj.", ".proj.base_layer.").replace(".fc1.", ".fc1.base_layer.")
             .replace(".fc2.", ".fc2.base_layer.") for n, _ in arch.PatchViT(**TINY).blocks[1].named_parameters()}
    assert set(state) == names
    ref = _tiny().state_dict()
    assert any(not torch.equal(v.to(DEV), ref[k.replace(".base_layer", "")]) for k, v in state.items())      # they were trained


def test_zz_report_error_to_bound_ratios():
    """Not a check of its own: prints the largest error / bound ratio every test above saw (each was asserted <= 1 there)."""
    for k in sorted(RATIOS):
        print(f"lora error/bound  {k:34s} {RATIOS[k]:.4f}")
    assert all(v <= 1.0 for v in RATIOS.values())
