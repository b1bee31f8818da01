"""Attention rollout without a device: the exported entry points and their shape limits, host-side argument checks of
ops.attention_rollout_step, PatchViT.attention_rollout and rollout_grid, the float64 oracle (the vector chain the code uses against the
explicit matrix product, mass conservation, a bound that is not vacuous) and the monitor CLIs' new flags."""
import importlib.util
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT

import _attention_rollout_oracle as RL
from oracle import attention_bounds as AB


def test_library_exports_the_three_entry_points():
    from dinox import _lib
    for name in ("dinox_attention_rollout_step_ok", "dinox_attention_rollout_step_ws_bytes", "dinox_attention_rollout_step"):
        assert hasattr(_lib.lib, name), name
    assert _lib.lib.dinox_version() == 3                                            # additive: the ABI number stays
    header = open(os.path.join(ROOT, "include", "dinox.h")).read()
    for name in ("int    dinox_attention_rollout_step_ok", "size_t dinox_attention_rollout_step_ws_bytes", "int    dinox_attention_rollout_step("):
        kind, sym = name.split()
        assert f"{kind} {sym}" in header, name


def test_ok_accepts_the_shipped_shapes_and_the_entry_rejects_the_rest_before_any_launch():
    from dinox import _lib
    L = _lib.lib
    # T = 257 (+ 4 registers) at d = 64 and d = 88, T = 1370 (+ 4) at d = 64, small odd shapes, the limits
    for good in ((32, 257, 6, 64), (32, 261, 6, 64), (8, 257, 16, 88), (8, 261, 16, 88), (1, 1370, 16, 64), (1, 1374, 16, 64), (1, 1, 1, 1),
                 (3, 5, 7, 3), (2, 63, 2, 16), (1, 4096, 1, 256)):
        assert L.dinox_attention_rollout_step_ok(*good) == 1, good
    assert L.dinox_attention_rollout_step_ws_bytes(2, 5, 3) == 2 * 5 * 3 * 4
    assert L.dinox_attention_rollout_step_ws_bytes(1, 1374, 16) == 1374 * 16 * 4
    assert L.dinox_attention_rollout_step_ws_bytes(0, 5, 3) == 0
    for bad in ((0, 5, 2, 8), (1, 0, 2, 8), (1, 5, 0, 8), (1, 5, 2, 0), (1, 5, 2, 257), (1, 4097, 2, 8), (1 << 20, 5, 1 << 12, 8)):
        assert L.dinox_attention_rollout_step_ok(*bad) == 0, bad
        assert L.dinox_attention_rollout_step(0x1000, 0x2000, 0x3000, 0x4000, *bad, 0.5, _lib.F32, None) == -1, bad
        assert "attention_rollout_step" in _lib.last_error()
    ok = (1, 5, 2, 8)
    assert L.dinox_attention_rollout_step(None, 0x2000, 0x3000, 0x4000, *ok, 0.5, _lib.F32, None) == -1 and "null pointer" in _lib.last_error()
    assert L.dinox_attention_rollout_step(0x1000, 0x2000, 0x3000, None, *ok, 0.5, _lib.F32, None) == -1 and "null pointer" in _lib.last_error()
    assert L.dinox_attention_rollout_step(0x1000, 0x2000, 0x3000, 0x4000, *ok, 0.5, 7, None) == -1 and "dtype" in _lib.last_error()
    for r in (-0.01, 1.5, float("nan")):
        assert L.dinox_attention_rollout_step(0x1000, 0x2000, 0x3000, 0x4000, *ok, r, _lib.F32, None) == -1 and "residual" in _lib.last_error()
    assert L.dinox_attention_rollout_step(0x1000, 0x2000, 0x2000, 0x4000, *ok, 0.5, _lib.F32, None) == -1 and "alias" in _lib.last_error()
    assert L.dinox_attention_rollout_step(0x1000, 0x2000, 0x2004, 0x4000, *ok, 0.5, _lib.F32, None) == -1 and "alias" in _lib.last_error()


def test_ops_argument_validation():
    """Every check is on the host and comes BEFORE the device is touched: ValueError, no launch."""
    from dinox import ops
    with pytest.raises(ValueError, match="device"):
        ops.attention_rollout_step(torch.zeros(2, 5, 48), 2, torch.zeros(2, 5))
    with pytest.raises(ValueError):
        ops.attention_rollout_step(torch.empty(2, 5, 48, device="meta"), 2, torch.zeros(2, 5))

    class OnDevice(torch.Tensor):                              # a host tensor that claims to live on the device: reaches the shape checks
        is_cuda = True

    def dev(*shape, dtype=torch.float32):
        return torch.zeros(*shape, dtype=dtype).as_subclass(OnDevice)

    q, w = dev(2, 5, 48), torch.zeros(2, 5)
    with pytest.raises(ValueError, match="float32 or bfloat16"):
        ops.attention_rollout_step(dev(2, 5, 48, dtype=torch.float16), 2, w)
    with pytest.raises(ValueError, match=r"\[B, N, 3 heads d\]"):
        ops.attention_rollout_step(dev(5, 48), 2, w)
    with pytest.raises(ValueError, match="5-D"):
        ops.attention_rollout_step(dev(2, 5, 3, 4, 4), 2, w)
    with pytest.raises(ValueError, match="heads=5"):
        ops.attention_rollout_step(q, 5, w)
    with pytest.raises(ValueError, match="heads=0"):
        ops.attention_rollout_step(q, 0, w)
    with pytest.raises(ValueError, match="head size 257"):
        ops.attention_rollout_step(dev(1, 2, 3 * 257), 1, torch.zeros(1, 2))
    with pytest.raises(ValueError, match="4097 tokens"):
        ops.attention_rollout_step(dev(1, 4097, 3), 1, torch.zeros(1, 4097))
    for bad_w in (torch.zeros(2, 4), torch.zeros(5), torch.zeros(2, 5, 1), torch.zeros(2, 5, dtype=torch.int64), [0.0] * 5):
        with pytest.raises(ValueError, match="w must be"):
            ops.attention_rollout_step(q, 2, bad_w)
    for r in (-0.1, 1.01, float("nan"), "0.5", None, True):
        with pytest.raises(ValueError, match="residual"):
            ops.attention_rollout_step(q, 2, w, residual=r)


def test_model_surface_rejects_bad_arguments_on_the_host():
    import zoo.arch as arch
    vit = arch.PatchViT(img_size=28, patch=14, dim=16, depth=2, heads=2, num_registers=1)
    x = torch.zeros(1, 3, 28, 28)
    for start in (2, -1, 1.0, True):
        with pytest.raises(ValueError, match="start_layer"):
            vit.attention_rollout(x, start_layer=start)
    for q in (6, -1, 0.0):                                                          # T = 1 + 4 + 1
        with pytest.raises(ValueError, match="query_token"):
            vit.attention_rollout(x, query_token=q)
    for r in (-0.5, 1.5, "x"):
        with pytest.raises(ValueError, match="residual"):
            vit.attention_rollout(x, residual=r)
    with pytest.raises(ValueError, match="at least one image"):
        vit.attention_rollout(x[:0])
    with pytest.raises((RuntimeError, ValueError)):             # CPU tensors: no CPU compute path
        vit.attention_rollout(x)


@pytest.mark.parametrize("registers", [0, 2])
def test_rollout_grid_shapes_and_errors(registers):
    from zoo.arch import rollout_grid
    B, P = 3, 16
    T = 1 + P + registers
    roll = torch.softmax(torch.randn(B, T, generator=torch.Generator().manual_seed(5), dtype=torch.float64), -1)
    grid = rollout_grid(roll, P)
    assert grid.shape == (B, 4, 4)
    assert torch.equal(grid.reshape(B, P), roll[:, 1:1 + P]) and torch.equal(grid[2, 3, 1], roll[2, 1 + 3 * 4 + 1])
    left_out = roll[:, 0] + roll[:, 1 + P:].sum(-1)                                 # CLS and register mass, exactly
    assert torch.allclose(1.0 - grid.sum((-1, -2)), left_out, rtol=0, atol=1e-15)
    for bad in ((roll, 15), (roll[:, :10], 16), (roll[0], 16), (roll[:, None], 16), (roll, 0)):
        with pytest.raises(ValueError):
            rollout_grid(*bad)


@pytest.mark.parametrize("case", AB.FAMILIES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_chain_is_the_explicit_product_and_conserves_mass(case, dtype):
    B, N, heads, d, L = 2, 19, 3, 8, 4
    blocks = [AB.make_qkv(case if l % 2 == 0 else "randn", B, N, heads, d, seed=30 + l, dtype=dtype) for l in range(L)]
    for residual in (0.0, 0.5, 1.0):
        for query in (0, N - 1):
            for start in (0, L - 1):
                chain = RL.chain_oracle(blocks[start:], heads, query, residual)
                explicit = RL.rollout_oracle(blocks[start:], heads, query, residual)
                assert chain["out"].shape == explicit.shape == (B, N)
                assert float((chain["out"] - explicit).abs().max()) <= 1e-12
                assert float((chain["out"].sum(-1) - 1.0).abs().max()) <= 1e-12 and bool((chain["out"] >= 0).all())
                assert 0.0 < chain["rho"] < 1e-2 and bool((chain["bound"] > 0).all())
    e = torch.zeros(B, N, dtype=torch.float64)
    e[:, 3] = 1.0
    assert torch.equal(RL.chain_oracle(blocks, heads, 3, 1.0)["out"], e)               # residual 1: the identity


def test_step_oracle_mass_linearity_and_a_bound_that_sees_errors():
    B, N, heads, d = 2, 33, 2, 16
    qkv = AB.make_qkv("ramp", B, N, heads, d, seed=3, dtype=torch.float32)
    g = torch.Generator().manual_seed(1)
    w = torch.rand(B, N, generator=g)
    w[:, ::3] = 0.0
    signed = torch.randn(B, N, generator=g)
    for r in (0.0, 0.5, 1.0):
        st = RL.step_oracle(qkv, heads, w, r)
        assert float((st["out"].sum(-1) - w.double().sum(-1)).abs().max()) <= 1e-12       # columns of a softmax row sum to 1
        a, b = RL.step_oracle(qkv, heads, signed, r), RL.step_oracle(qkv, heads, 2.0 * signed, r)
        assert torch.allclose(2.0 * a["out"], b["out"], rtol=1e-13, atol=0) and torch.allclose(2.0 * (a["bound"] - RL.TINY), b["bound"] - RL.TINY, rtol=1e-12, atol=0)
        assert RL.check(st["out"], st["out"], st["bound"], "oracle") == 0.0
        # not below the output format: rounding to fp32 costs 2^-24 of r |w| + the attention term, the bound grants 2^-23 r |w| + ...
        assert 0.0 <= RL.check(st["out"].float(), st["out"], st["bound"], "oracle in fp32") <= 0.5
    st = RL.step_oracle(qkv, heads, w, 0.5)
    P, _ = RL.softmax_matrices(qkv, heads)
    dropped = st["out"] - 0.5 / heads * w.double()[:, 1:2] * P[:, 0, 1, :]              # one query row of one head left out
    with pytest.raises(AssertionError):
        RL.check(dropped, st["out"], st["bound"], "dropped row")
    with pytest.raises(AssertionError):
        RL.check(st["out"].roll(1, -1), st["out"], st["bound"], "shifted keys")
    # one-hot w, residual 0: the head mean of that softmax row
    e = torch.zeros(B, N)
    e[:, 7] = 1.0
    assert torch.allclose(RL.step_oracle(qkv, heads, e, 0.0)["out"], P[:, :, 7].mean(1), rtol=1e-14, atol=0)


def _load_script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "dino-x_amd", "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def test_monitor_cli_flag():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "dino-x_amd", "scripts", "phase5_monitor.py"), "--help"], capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0 and "--rollout" in out.stdout
    mon = _load_script("phase5_monitor")
    assert mon.build_parser().parse_args(["--checkpoint", "x.pth"]).rollout is False
    assert mon.build_parser().parse_args(["--checkpoint", "x.pth", "--rollout"]).rollout is True


def test_run_monitor_has_the_opt_in_argument():
    import inspect
    from dinox.monitor import run_monitor
    p = inspect.signature(run_monitor).parameters["rollout"]
    assert p.default is False
