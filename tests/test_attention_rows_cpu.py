"""Attention rows and the monitor without a device: the float64 oracle against the full softmax on every adversarial input family,
the CLS-grid indexing, the monitor's heatmap and statistics against values recorded from the reference (monitor_tiny.npz), host-side
argument checks of ops.attention_rows and of the two CLIs."""
import importlib.util
import math
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

import _attention_rows_oracle as RO
from oracle import attention_bounds as AB

QUERIES = [(0,), (0, 16), (3, 3, 0, 16, 9, 1, 2, 5), (16,)]


@pytest.mark.parametrize("case", AB.FAMILIES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_oracle_rows_equal_the_full_softmax(case, dtype):
    B, N, heads, d = 2, 17, 3, 16
    qkv = AB.make_qkv(case, B, N, heads, d, seed=11, dtype=dtype)
    for idx in QUERIES:
        ref = RO.rows_oracle(qkv, heads, idx)
        full = RO.full_softmax_rows(qkv, heads, idx)
        assert ref["probs"].shape == (B, heads, len(idx), N) and ref["lse"].shape == (B, heads, len(idx))
        assert torch.allclose(ref["probs"], full, rtol=1e-12, atol=1e-300)
        assert torch.allclose(ref["probs"].sum(-1), torch.ones(B, heads, len(idx), dtype=torch.float64), rtol=0, atol=1e-13)
        # the oracle satisfies its own bound (trivially), and so does an fp32 rounding of it: the bound is not below the output format
        r = RO.check_rows(ref["probs"], ref["lse"], ref, f"{case} oracle")
        assert r == {"p": 0.0, "sum": r["sum"], "lse": 0.0} and r["sum"] < 1e-6
        r32 = RO.check_rows(ref["probs"].float(), ref["lse"].float(), ref, f"{case} oracle in fp32")
        assert 0.0 < r32["p"] < 0.1 and r32["lse"] < 0.1
        # ... and it is not vacuous: one key dropped from the normaliser of a uniform-ish row would be seen
        assert float(ref["lse_bound"].max()) <= 1.0 / (2 * N)


def test_oracle_bound_sees_a_wrong_row():
    qkv = AB.make_qkv("randn", 1, 65, 1, 16, seed=3, dtype=torch.float32)
    ref = RO.rows_oracle(qkv, 1, (0, 64))
    wrong = ref["probs"].clone()
    wrong[0, 0, 1] = ref["probs"][0, 0, 0]                   # row of token 64 replaced by the row of token 0
    with pytest.raises(AssertionError, match="probs"):
        RO.check_rows(wrong, None, ref, "swapped")
    dropped = ref["probs"].clone()
    dropped[..., 64] = 0.0                                    # the last key (a lane of the second wave) left out
    with pytest.raises(AssertionError):
        RO.check_rows(dropped, None, ref, "dropped key")


@pytest.mark.parametrize("registers", [0, 2])
def test_cls_attention_grid_indexing(registers):
    from zoo.arch import cls_attention_grid
    B, heads, Q, P = 2, 3, 2, 16
    T = 1 + P + registers
    g = torch.Generator().manual_seed(5)
    probs = torch.softmax(torch.randn(B, heads, Q, T, generator=g, dtype=torch.float64), -1)
    grid = cls_attention_grid(probs, P)
    assert grid.shape == (B, heads, 4, 4)
    assert torch.equal(grid.reshape(B, heads, P), probs[:, :, 0, 1:1 + P])          # row 0, patch columns, row-major grid
    assert torch.equal(grid[1, 2, 3, 1], probs[1, 2, 0, 1 + 3 * 4 + 1])
    left_out = probs[:, :, 0, 0] + probs[:, :, 0, 1 + P:].sum(-1)                   # CLS and register mass, exactly
    assert torch.allclose(1.0 - grid.sum((-1, -2)), left_out, rtol=0, atol=1e-15) and bool((grid.sum((-1, -2)) < 1).all())
    with pytest.raises(ValueError):
        cls_attention_grid(probs, 15)
    with pytest.raises(ValueError):
        cls_attention_grid(probs[..., :10], 16)


def test_monitor_heatmap_and_stats_match_the_reference_fixture():
    from dinox.monitor import attention_entropy, embedding_stats, patch_norm_heatmap
    g = load_golden("monitor_tiny.npz")
    feats = torch.from_numpy(g["feats"])
    assert feats.shape == (8, 1 + 16 + 2, 64) and g["heatmap"].shape == (8, 4, 4)
    heat = patch_norm_heatmap(feats, 16)
    assert heat.shape == (8, 4, 4) and heat.dtype == torch.float32
    np.testing.assert_allclose(heat.numpy(), g["heatmap"], rtol=1e-6, atol=1e-7)
    assert float(heat.amin()) == 0.0 and 0.999 < float(heat.amax()) <= 1.0
    st = embedding_stats(feats[:, 0])
    assert set(st) == {"embedding_std_mean", "embedding_norm_mean"}
    assert abs(st["embedding_std_mean"] - float(g["embedding_std_mean"])) <= 1e-6 * float(g["embedding_std_mean"])
    assert abs(st["embedding_norm_mean"] - float(g["embedding_norm_mean"])) <= 1e-6 * float(g["embedding_norm_mean"])
    with pytest.raises(ValueError):
        patch_norm_heatmap(feats, 15)
    with pytest.raises(ValueError):
        embedding_stats(feats)
    # entropy: log T for a uniform row, 0 for a one-hot row (0 log 0 = 0)
    T = 19
    rows = torch.stack([torch.full((T,), 1.0 / T), torch.eye(T)[4]])
    ent = attention_entropy(rows)
    assert abs(float(ent[0]) - math.log(T)) < 1e-6 and float(ent[1]) == 0.0


def test_first_images_of_a_tensor_and_of_a_patch_operand():
    from dinox import ops
    from dinox.monitor import first_images
    from oracle.kernels_np import unfold_patches
    g = torch.Generator().manual_seed(2)
    x = torch.randn(5, 3, 28, 28, generator=g)
    sub, plane = first_images(x, 32)
    assert sub.shape == (5, 3, 28, 28) and torch.equal(plane, x[0, 1])
    assert first_images(x, 2)[0].shape[0] == 2
    u = torch.from_numpy(unfold_patches(x.numpy(), 14).reshape(5 * 4, -1))
    u = torch.cat([u, torch.zeros(20, 4)], 1)                 # padded columns, as the operand of the 14-pixel patch carries
    sub, plane = first_images(ops.PatchOperand(u, 5, 28, 14), 3)
    assert isinstance(sub, ops.PatchOperand) and sub.shape == (3, 3, 28, 28) and sub.u.data_ptr() == u.data_ptr() and sub.u.shape[0] == 12
    assert torch.equal(plane, x[0, 1])


def test_attention_rows_argument_validation():
    """Every check is on the host and comes BEFORE the device is touched: ValueError, no launch."""
    from dinox import ops
    cpu = torch.zeros(2, 5, 3 * 2 * 8)
    with pytest.raises(ValueError, match="device"):
        ops.attention_rows(cpu, 2, (0,))
    fake = torch.empty(2, 5, 3 * 2 * 8, device="meta")        # is_cuda False as well: the device check comes first
    with pytest.raises(ValueError):
        ops.attention_rows(fake, 2, (0,))

    class OnDevice(torch.Tensor):                              # a host tensor that claims to live on the device: reaches the shape checks
        is_cuda = True

    def dev(*shape, dtype=torch.float32):
        return torch.zeros(*shape, dtype=dtype).as_subclass(OnDevice)

    q = dev(2, 5, 48)
    with pytest.raises(ValueError, match=r"outside \[0, 5\)"):
        ops.attention_rows(q, 2, (0, 5))
    with pytest.raises(ValueError, match=r"outside \[0, 5\)"):
        ops.attention_rows(q, 2, (-1,))
    with pytest.raises(ValueError, match="1 to 8 query rows"):
        ops.attention_rows(q, 2, ())
    with pytest.raises(ValueError, match="1 to 8 query rows"):
        ops.attention_rows(q, 2, tuple(range(5)) + tuple(range(4)))
    with pytest.raises(ValueError, match=r"\[B, N, 3 heads d\]"):
        ops.attention_rows(dev(5, 48), 2, (0,))
    with pytest.raises(ValueError, match=r"\[B, N, 3 heads d\]"):
        ops.attention_rows(dev(2, 5, 3, 16), 2, (0,))
    with pytest.raises(ValueError, match="5-D"):
        ops.attention_rows(dev(2, 5, 3, 4, 4), 2, (0,))
    with pytest.raises(ValueError, match="heads=5"):
        ops.attention_rows(q, 5, (0,))
    with pytest.raises(ValueError, match="float32 or bfloat16"):
        ops.attention_rows(dev(2, 5, 48, dtype=torch.float16), 2, (0,))
    with pytest.raises(ValueError, match="head size 257"):
        ops.attention_rows(dev(1, 2, 3 * 257), 1, (0,))
    with pytest.raises(ValueError, match="integers"):
        ops.attention_rows(q, 2, (0.5,))
    with pytest.raises(ValueError, match="1-D int32 / int64"):
        ops.attention_rows(q, 2, torch.zeros(1, 1, dtype=torch.int64))


def test_attention_rows_c_entry_rejects_bad_arguments_before_any_launch():
    from dinox import _lib
    L = _lib.lib
    assert L.dinox_attention_rows_ok(1, 1, 1, 1, 1) == 1 and L.dinox_attention_rows_ok(32, 1374, 16, 256, 8) == 1
    for bad in ((0, 5, 2, 8, 1), (1, 0, 2, 8, 1), (1, 5, 0, 8, 1), (1, 5, 2, 0, 1), (1, 5, 2, 257, 1), (1, 5, 2, 8, 0), (1, 5, 2, 8, 9),
                (1 << 20, 5, 1 << 12, 8, 1)):
        assert L.dinox_attention_rows_ok(*bad) == 0, bad
        assert L.dinox_attention_rows(0x1000, 0x2000, 0x3000, None, *bad, _lib.F32, None) == -1, bad
        assert "attention_rows" in _lib.last_error()
    assert L.dinox_attention_rows(None, 0x2000, 0x3000, None, 1, 5, 2, 8, 1, _lib.F32, None) == -1 and "null pointer" in _lib.last_error()
    assert L.dinox_attention_rows(0x1000, 0x2000, 0x3000, None, 1, 5, 2, 8, 1, 7, None) == -1 and "dtype" in _lib.last_error()


def test_last_attention_rejects_bad_arguments_on_the_host():
    import zoo.arch as arch
    vit = arch.PatchViT(img_size=28, patch=14, dim=16, depth=2, heads=2, num_registers=1)
    x = torch.zeros(1, 3, 28, 28)
    for layer in (2, -3, 1.0):
        with pytest.raises(ValueError, match="layer"):
            vit.last_attention(x, layer=layer)
    with pytest.raises(ValueError, match="at least one image"):
        vit.last_attention(x[:0])
    with pytest.raises((RuntimeError, ValueError)):             # CPU tensors: no CPU compute path
        vit.last_attention(x)


def _load_script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "dino-x_amd", "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def test_monitor_cli_host_side_argument_errors(tmp_path):
    mon = _load_script("phase5_monitor")
    flags = {a.option_strings[0] for a in mon.build_parser()._actions if a.option_strings}
    assert {"--checkpoint", "--index-csv", "--synthetic", "--fixed-png", "--sample-seed", "--level", "--width", "--batch-size", "--out-dir",
            "--scale-aware", "--amp"} <= flags
    d = mon.build_parser().parse_args(["--checkpoint", "x.pth"])
    assert (d.level, d.width, d.batch_size, d.sample_seed, d.synthetic) == (-600.0, 1500.0, 32, 42, 0)
    with pytest.raises(SystemExit):
        mon.main([])                                                               # --checkpoint is required
    with pytest.raises(FileNotFoundError, match="Checkpoint not found"):
        mon.main(["--checkpoint", str(tmp_path / "none.pth"), "--synthetic", "8"])
    ck = tmp_path / "c.pth"
    ck.write_bytes(b"")
    with pytest.raises(FileNotFoundError, match="index_csv not found"):
        mon.main(["--checkpoint", str(ck), "--index-csv", str(tmp_path / "none.csv")])
    with pytest.raises(SystemExit, match="--synthetic must be >= 0"):
        mon.main(["--checkpoint", str(ck), "--synthetic", "-1"])
    with pytest.raises(SystemExit, match="--batch-size must be > 0"):
        mon.main(["--checkpoint", str(ck), "--synthetic", "8", "--batch-size", "0"])
    with pytest.raises(SystemExit, match="--width must be > 0"):
        mon.main(["--checkpoint", str(ck), "--synthetic", "8", "--width", "0"])
    with pytest.raises(SystemExit, match="not with --synthetic"):
        mon.main(["--checkpoint", str(ck), "--synthetic", "8", "--fixed-png", "a.png"])
    if not torch.cuda.is_available():
        with pytest.raises(SystemExit, match="computes on MI355X only"):
            mon.main(["--checkpoint", str(ck), "--synthetic", "8"])


def test_training_cli_monitor_every_reaches_the_config(cli):
    args = cli.build_parser().parse_args(["--monitor-every", "0", "--synthetic", "8"])
    assert args.monitor_every == 0
    assert cli.build_parser().parse_args([]).monitor_every == 1000                 # the reference's default is kept
    assert cli.TrainingConfig.__dataclass_fields__["monitor_every"].default == 1000
    cfg = cli.TrainingConfig(model=cli.ModelConfig("custom", 16, 64, 2, 2), hardware=cli.HardwareConfig("cuda", "x", True, 0, False, 64), monitor_every=args.monitor_every)
    assert cfg.monitor_every == 0 and cli.asdict(cfg)["monitor_every"] == 0
    assert "accepted and ignored" not in cli.__doc__ and "--monitor-every" in cli.__doc__
    # the collapse guard the monitor feeds
    assert cli.detect_anomaly(0.0, [], embedding_std=0.001)[0] and not cli.detect_anomaly(0.0, [], embedding_std=0.5)[0]
