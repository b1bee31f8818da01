"""dinox_attention_rollout_step and the surfaces on it, on the device: every element of a step against the float64 oracle inside the
a-priori bound of tests/_attention_rollout_oracle.py (nothing masked or left out), the landed row kernel as a second witness, mass
conservation, bit reproducibility, the unaligned load path, PatchViT.attention_rollout against the explicit matrix product,
zoo.encode.attention_rollout, and a monitor that writes the rollout on request and leaves training bit-identical.

The bound tests print their largest err / bound ratio per case (run with -s)."""
import json

import numpy as np
import pytest
import torch

import _attention_rollout_oracle as RL
import _attention_rows_oracle as RO
from oracle import attention_bounds as AB

pytestmark = pytest.mark.gpu

DEV = "cuda"
# (B, N, heads, d).  N: one key; under, at and over one wave; under one 256-thread stride (201: ViT-S/16 at 224) and over it (261:
# ViT-g/14 at 224 with registers); N % 8 takes every remainder class that matters (1, 7, 0, 1, 1, 5).  d: 8 / 16 / 64 take the 16-byte
# loads in both dtypes, 24 and 88 in both too (multiples of 8), which leaves the scalar path to the unaligned test and to d = 7, 12.
SHAPES = ((1, 1, 1, 8), (2, 63, 2, 16), (2, 64, 3, 64), (3, 65, 2, 24), (1, 201, 6, 64), (1, 261, 2, 88), (2, 21, 2, 7), (1, 37, 3, 12))
RESIDUALS = (0.0, 0.5, 1.0)


@pytest.fixture(scope="module")
def dx():
    from dinox import ops
    import zoo.arch as arch
    import dinox._lib as L
    assert L.lib.dinox_device_ok() == 1, L.last_error()
    return ops, arch


def weights(B, N, seed):
    """Random non-negative, the same with zeros in it (single zeros, a whole chunk of 8 rows, the tail), and signed."""
    g = torch.Generator().manual_seed(seed)
    pos = torch.rand(B, N, generator=g)
    holes = pos.clone()
    holes[:, ::3] = 0.0
    holes[:, 8:16] = 0.0
    holes[:, N - (N // 4):] = 0.0
    return {"nonneg": pos, "zeros": holes, "signed": torch.randn(B, N, generator=g)}


def run_step(ops, qkv, heads, w, residual, what):
    ref = RL.step_oracle(qkv, heads, w, residual)
    out = ops.attention_rollout_step(qkv.to(DEV), heads, w.to(DEV), residual)
    assert out.shape == w.shape and out.dtype == torch.float32 and not out.requires_grad
    return RL.check(out, ref["out"], ref["bound"], what), out, ref


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", AB.FAMILIES)
def test_step_inside_the_bound_elementwise(dx, case, dtype):
    ops, _ = dx
    worst = 0.0
    for n, (B, N, heads, d) in enumerate(SHAPES):
        qkv = AB.make_qkv(case, B, N, heads, d, seed=200 + n, dtype=dtype)
        for name, w in weights(B, N, 300 + n).items():
            for r in RESIDUALS:
                ratio, out, _ = run_step(ops, qkv, heads, w, r, f"{case} {dtype} B={B} N={N} heads={heads} d={d} w={name} residual={r}")
                worst = max(worst, ratio)
                if r == 1.0:
                    assert torch.equal(out.cpu(), w)                                   # the identity, exactly
    print(f"attention_rollout_step {case} {dtype}: largest err / bound {worst:.4f}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", ["randn", "ramp"])
def test_step_at_518_pixel_token_count(dx, case, dtype):
    """N = 1370 (518 px at patch 14): six keys per thread, 172 chunks of query rows, a ragged last chunk and a ragged last stride."""
    ops, _ = dx
    B, N, heads, d = 1, 1370, 1, 64
    qkv = AB.make_qkv(case, B, N, heads, d, seed=21, dtype=dtype)
    ratio, _, _ = run_step(ops, qkv, heads, weights(B, N, 22)["zeros"], 0.5, f"N=1370 {case} {dtype}")
    print(f"attention_rollout_step N=1370 {case} {dtype}: largest err / bound {ratio:.4f}")


def test_step_past_64_kib_of_lds(dx):
    """N = 2049: the chunk's score rows pass 64 KiB of LDS (the launch raises the kernel's limit first) and a thread owns nine keys."""
    ops, _ = dx
    B, N, heads, d = 1, 2049, 1, 8
    qkv = AB.make_qkv("randn", B, N, heads, d, seed=23, dtype=torch.bfloat16)
    w = torch.zeros(B, N)
    w[:, [0, 5, 1030, 2040, 2048]] = torch.tensor([0.5, 0.25, 1.0, 0.125, 2.0])      # five chunks of 257 do the work
    ratio, _, _ = run_step(ops, qkv, heads, w, 0.25, "N=2049")
    print(f"attention_rollout_step N=2049: largest err / bound {ratio:.4f}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_one_hot_step_is_the_head_mean_of_the_row_kernel(dx, dtype):
    """w = e_i, residual 0: row i of mean_h P^h, which dinox_attention_rows computes on its own.  Each kernel is inside its own bound
    of float64, so the two agree within the sum of the bounds."""
    ops, _ = dx
    for case, (B, N, heads, d) in (("randn", (2, 65, 3, 24)), ("offset", (1, 201, 6, 64)), ("onehot", (2, 63, 2, 16))):
        qkv = AB.make_qkv(case, B, N, heads, d, seed=31, dtype=dtype)
        dq = qkv.to(DEV)
        for i in (0, N // 2, N - 1):
            w = torch.zeros(B, N)
            w[:, i] = 1.0
            _, out, ref = run_step(ops, qkv, heads, w, 0.0, f"one-hot {case} row {i}")
            rows = ops.attention_rows(dq, heads, (i,))                                   # [B, heads, 1, N]
            rref = RO.rows_oracle(qkv, heads, (i,))
            RO.check_rows(rows, None, rref, f"rows {case} row {i}")
            mean = rows[:, :, 0].double().cpu().mean(1)
            tol = ref["bound"] + rref["p_bound"][:, :, 0].mean(1)
            diff = (out.double().cpu() - mean).abs()
            assert bool((diff <= tol).all()), f"{case} row {i}: kernels differ by {float(diff.max()):.3e}, tolerance {float(tol[diff.argmax() // N, diff.argmax() % N]):.3e}"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_mass_is_conserved(dx, dtype):
    """sum_j out_j = sum_j w_j for a non-negative w (every softmax row sums to 1), within the summed bound."""
    ops, _ = dx
    for n, (B, N, heads, d) in enumerate(SHAPES):
        for case in ("randn", "lastkey"):
            qkv = AB.make_qkv(case, B, N, heads, d, seed=40 + n, dtype=dtype)
            for name in ("nonneg", "zeros"):
                w = weights(B, N, 50 + n)[name]
                for r in (0.0, 0.5):
                    _, out, ref = run_step(ops, qkv, heads, w, r, f"mass {case} {name}")
                    diff = (out.double().cpu().sum(-1) - w.double().sum(-1)).abs()
                    assert bool((diff <= ref["bound"].sum(-1)).all()), (case, name, r, diff, ref["bound"].sum(-1))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_bit_reproducible_and_layouts(dx, dtype):
    ops, _ = dx
    B, N, heads, d = 3, 261, 3, 64
    qkv = AB.make_qkv("randn", B, N, heads, d, seed=9, dtype=dtype).to(DEV)
    w = weights(B, N, 10)["signed"].to(DEV)
    a = ops.attention_rollout_step(qkv, heads, w, 0.5)
    assert torch.equal(a, ops.attention_rollout_step(qkv, heads, w, 0.5))
    assert torch.equal(a, ops.attention_rollout_step(qkv.view(B, N, 3, heads, d), heads, w, 0.5))        # the 5-D form
    assert torch.equal(a, ops.attention_rollout_step(qkv, heads, w.double(), 0.5))                         # w is taken as fp32
    assert torch.equal(a[1:2], ops.attention_rollout_step(qkv[1:2], heads, w[1:2], 0.5))                   # an image does not see its neighbours
    assert not ops.attention_rollout_step(qkv.clone().requires_grad_(), heads, w, 0.5).requires_grad       # no gradient is defined
    ops.TRACE_KERNELS = []
    try:
        ops.attention_rollout_step(qkv, heads, w)
        assert ops.TRACE_KERNELS == ["attention_rollout_step"]
    finally:
        ops.TRACE_KERNELS = None
    with pytest.raises(ValueError, match="w must be"):
        ops.attention_rollout_step(qkv, heads, w[:, :-1])
    with pytest.raises(ValueError, match="device"):
        ops.attention_rollout_step(qkv, heads, w.cpu())
    torch.cuda.synchronize()


def test_unaligned_base_takes_the_scalar_path(dx):
    """A packed tensor that starts one element into its allocation is contiguous but not 16-byte aligned."""
    ops, _ = dx
    for dtype in (torch.float32, torch.bfloat16):
        B, N, heads, d = 2, 65, 2, 16
        qkv = AB.make_qkv("ramp", B, N, heads, d, seed=4, dtype=dtype)
        w = weights(B, N, 5)["signed"]
        buf = torch.empty(qkv.numel() + 1, dtype=dtype, device=DEV)
        view = buf[1:].view(qkv.shape)
        view.copy_(qkv)
        assert view.data_ptr() % 16 != 0 and view.is_contiguous()
        ref = RL.step_oracle(qkv, heads, w, 0.5)
        out = ops.attention_rollout_step(view, heads, w.to(DEV), 0.5)
        RL.check(out, ref["out"], ref["bound"], f"unaligned {dtype}")
        assert torch.equal(out, ops.attention_rollout_step(qkv.to(DEV), heads, w.to(DEV), 0.5))   # the two load paths add in the same order


# ------------------------------------------------------------------------------------------ model surface
def _tiny(arch, registers):
    return arch.PatchViT(img_size=32, patch=8, dim=64, depth=3, heads=2, num_registers=registers)


def _hooked(model, fn):
    """fn() with a forward hook on every block's qkv module -> (fn's result, the products in block order)."""
    got = {}
    hooks = [b.attn.qkv.register_forward_hook(lambda m, i, o, k=k: got.setdefault(k, []).append(o.detach())) for k, b in enumerate(model.blocks)]
    try:
        res = fn()
    finally:
        for h in hooks:
            h.remove()
    return res, got


@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("registers", [0, 2])
def test_model_rollout(dx, registers, amp):
    ops, arch = dx
    torch.manual_seed(0)
    model = _tiny(arch, registers).to(DEV).eval()
    depth, heads, B, T = 3, 2, 2, 17 + registers
    x = torch.randn(B, 3, 32, 32, generator=torch.Generator().manual_seed(1)).to(DEV)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
        with torch.no_grad():
            want = model(x)
        (feats, roll), got = _hooked(model, lambda: model.attention_rollout(x))
        f_last, r_last = model.attention_rollout(x, start_layer=depth - 1, residual=0.25)
        (_, probs), got_last = _hooked(model, lambda: model.last_attention(x, query_tokens=(0,)))
        f_q, r_q = model.attention_rollout(x, query_token=T - 1, residual=0.0, start_layer=1)
    assert torch.equal(feats, want) and torch.equal(f_last, want) and torch.equal(f_q, want) and not feats.requires_grad
    assert roll.shape == (B, T) and roll.dtype == torch.float32 and not roll.requires_grad and not model.training
    assert sorted(got) == [0, 1, 2] and all(len(v) == 1 and v[0].shape == (B, T, 3 * 64) for v in got.values())
    assert all(v[0].dtype == (torch.bfloat16 if amp else torch.float32) for v in got.values())     # the current compute dtype
    blocks = [got[k][0].cpu() for k in range(depth)]

    # the explicit float64 product of the blocks' own matrices, within the composed bound (1 + rho)^L - 1
    chain = RL.chain_oracle(blocks, heads, 0, 0.5)
    explicit = RL.rollout_oracle(blocks, heads, 0, 0.5)
    bound = RL.chain_bound(explicit, chain["rho"], depth)
    ratio = RL.check(roll, explicit, bound, "rollout against the explicit product")
    # it sums to 1 within the summed bound
    assert bool(((roll.double().cpu().sum(-1) - 1.0).abs() <= bound.sum(-1)).all())
    # another query token, no residual, two blocks
    explicit_q = RL.rollout_oracle(blocks[1:], heads, T - 1, 0.0)
    RL.check(r_q, explicit_q, RL.chain_bound(explicit_q, chain["rho"], depth - 1), "rollout of the last token over two blocks")

    # the same product from the landed row kernel, 8 query rows at a time: both kernels are inside (1 + rho)^L - 1 of float64
    R = None
    for qkv in blocks:
        rows = torch.cat([ops.attention_rows(qkv.to(DEV), heads, tuple(range(i, min(i + 8, T)))) for i in range(0, T, 8)], 2)   # [B, heads, T, T]
        Ahat = 0.5 * torch.eye(T, dtype=torch.float64) + 0.5 * rows.double().cpu().mean(1)
        R = Ahat if R is None else Ahat @ R
    diff = (roll.double().cpu() - R[:, 0]).abs()
    assert bool((diff <= 2.0 * bound).all()), f"rollout and the row kernel's product differ by {float(diff.max()):.3e}"

    # start_layer = depth - 1: residual e_0 + (1 - residual) head mean of last_attention's row, within the sum of the two bounds
    last = got_last[depth - 1][0].cpu()
    assert torch.equal(last, blocks[-1])
    e0 = torch.zeros(B, T)
    e0[:, 0] = 1.0
    st = RL.step_oracle(last, heads, e0, 0.25)
    RL.check(r_last, st["out"], st["bound"], "start_layer = depth - 1")
    expect = 0.25 * e0.double() + 0.75 * probs[:, :, 0].double().cpu().mean(1)
    tol = st["bound"] + 0.75 * RO.rows_oracle(last, heads, (0,))["p_bound"][:, :, 0].mean(1)
    assert bool(((r_last.double().cpu() - expect).abs() <= tol).all())
    print(f"model rollout registers={registers} amp={amp}: largest err / bound {ratio:.4f}")


def test_encode_attention_rollout(dx):
    ops, arch = dx
    from zoo.encode import attention_rollout, encode, _batch
    torch.manual_seed(0)
    vit = arch.PatchViT(img_size=32, patch=8, dim=64, depth=3, heads=2, scale_aware=True).to(DEV).eval()
    img = np.random.default_rng(0).uniform(-1000, 1000, size=(48, 40)).astype(np.float32)
    m = attention_rollout(vit, img, (0.7, 0.7), 2.5)
    assert isinstance(m, np.ndarray) and m.shape == (4, 4) and m.dtype == np.float32
    assert np.isfinite(m).all() and (m >= 0).all() and 0.0 < m.sum() <= 1.0
    x = _batch([img], 32, "hu_float", 40.0, 400.0, DEV, "host")
    _, roll = vit.attention_rollout(x, torch.tensor([[0.7, 0.7, 2.5]], device=DEV))
    assert np.array_equal(m, arch.rollout_grid(roll, 16)[0].cpu().numpy())
    m1 = attention_rollout(vit, img, residual=0.0, start_layer=2)
    assert m1.shape == (4, 4) and not np.array_equal(m1, attention_rollout(vit, img))
    assert attention_rollout(vit, img, preprocess="auto").shape == (4, 4)
    with pytest.raises(ValueError, match="Unknown input_format"):
        attention_rollout(vit, img, input_format="nope")
    with pytest.raises(ValueError, match="start_layer"):
        attention_rollout(vit, img, start_layer=3)
    assert encode(vit, img).shape == (1, 1, 64)                                           # the existing surface is untouched


# ------------------------------------------------------------------------------------------ monitor
PARENT_FILES = {"heatmap.npy", "attention.npy", "input.npy", "stats.json", "heatmap.png", "input.png", "attention.png"}
PARENT_KEYS = {"step", "embedding_std_mean", "embedding_norm_mean", "attention_entropy", "attention_entropy_max", "attention_patch_mass", "batch"}


def test_run_monitor_writes_the_rollout_on_request_only(dx, tmp_path):
    ops, arch = dx
    from dinox.monitor import run_monitor
    try:
        import PIL  # noqa: F401
        pngs = True
    except Exception:
        pngs = False
    torch.manual_seed(0)
    vit = _tiny(arch, 2).to(DEV).eval()
    x = torch.randn(3, 3, 32, 32, generator=torch.Generator().manual_seed(2)).to(DEV)
    off = run_monitor(vit, x, None, tmp_path / "off", 7)
    on = run_monitor(vit, x, None, tmp_path / "on", 7, rollout=True)
    files = {n for n in PARENT_FILES if pngs or not n.endswith(".png")}
    assert {p.name for p in (tmp_path / "off" / "step_00000007").iterdir()} == files
    assert {p.name for p in (tmp_path / "on" / "step_00000007").iterdir()} == files | {"rollout.npy"} | ({"rollout.png"} if pngs else set())
    assert set(off) == PARENT_KEYS | {"dir"} and set(on) == PARENT_KEYS | {"dir", "rollout_patch_mass", "rollout_entropy"}
    st_off = json.loads((tmp_path / "off" / "step_00000007" / "stats.json").read_text())
    st_on = json.loads((tmp_path / "on" / "step_00000007" / "stats.json").read_text())
    assert set(st_off) == PARENT_KEYS and set(st_on) == PARENT_KEYS | {"rollout_patch_mass", "rollout_entropy"}
    assert all(st_on[k] == st_off[k] for k in PARENT_KEYS)                                # the rest does not move
    for name in ("heatmap", "attention", "input"):
        assert np.array_equal(np.load(tmp_path / "on" / "step_00000007" / f"{name}.npy"), np.load(tmp_path / "off" / "step_00000007" / f"{name}.npy"))
    r = np.load(tmp_path / "on" / "step_00000007" / "rollout.npy")
    _, roll = vit.attention_rollout(x)
    assert r.shape == (4, 4) and np.array_equal(r, arch.rollout_grid(roll, 16)[0].cpu().numpy())
    assert 0.0 < st_on["rollout_patch_mass"] < 1.0 and 0.0 <= st_on["rollout_entropy"] <= st_on["attention_entropy_max"] + 1e-5
    assert abs(st_on["rollout_patch_mass"] - float(roll[:, 1:17].sum(-1).mean())) <= 1e-6


@pytest.mark.parametrize("graph,amp", [(False, False), (True, False), (True, True)], ids=["eager", "graph", "graph-bf16"])
def test_monitor_rollout_leaves_the_training_state_bit_identical(dx, tmp_path, graph, amp):
    """Four steps with run_monitor(rollout=True) after steps 2 and 4 against four steps without any monitor.  With use_graph the first
    call falls between the last eager step and the capture, the second between two replays: the rollout's second forward and its chain
    are launched eagerly, outside the captured step."""
    ops, arch = dx
    from dinox.engine import StepHyperParams, TrainEngine
    from dinox.monitor import run_monitor
    kw = dict(img_size=32, patch=8, dim=64, depth=2, heads=2, num_registers=2, scale_aware=True)
    gen = torch.Generator().manual_seed(6)
    batches = [(torch.randn(4, 3, 32, 32, generator=gen).to(DEV), (torch.rand(4, 3, generator=gen) + 0.5).to(DEV)) for _ in range(4)]

    def run(monitor):
        torch.manual_seed(0)
        s_ = arch.DinoStudentTeacher(arch.PatchViT(**kw), 64)
        t_ = arch.DinoStudentTeacher(arch.PatchViT(**kw), 64)
        t_.load_state_dict(s_.state_dict())
        eng = TrainEngine(s_.to(DEV), t_.to(DEV), 64, StepHyperParams(lr=1e-3, warmup_steps=2, max_steps=10, ema=0.9), use_graph=graph,
                          amp_dtype=torch.bfloat16 if amp else None)
        out = []
        for i, (b, sp) in enumerate(batches):
            eng.step(b, sp)
            if monitor and (i + 1) % 2 == 0:
                with ops.compute_dtype(eng.compute_dtype):
                    out.append(run_monitor(s_.backbone, b, sp, tmp_path / "mon", i + 1, rollout=True))
        torch.cuda.synchronize()
        assert (eng._graph is not None) == graph
        return [t.clone() for t in (eng.flat_p, eng.flat_t, eng.center, eng.adam_m, eng.adam_v)], out

    plain, _ = run(False)
    watched, stats = run(True)
    for name, a, b in zip(("flat_p", "flat_t", "center", "adam_m", "adam_v"), plain, watched):
        assert torch.equal(a, b), name
    assert [s["step"] for s in stats] == [2, 4] and all(0.0 < s["rollout_patch_mass"] < 1.0 for s in stats)
    assert np.load(tmp_path / "mon" / "step_00000004" / "rollout.npy").shape == (4, 4)


def test_monitor_script_writes_the_rollout_of_a_checkpoint(dx, cli, tmp_path, capsys):
    """A 4-step tiny run leaves a checkpoint; scripts/phase5_monitor.py --rollout on it writes rollout.npy / rollout.png and the two
    stats keys, and without the flag exactly the earlier files and keys."""
    import importlib.util
    import os
    import sys
    cli.main(["--config", "custom", "--vit-patch", "16", "--vit-dim", "64", "--vit-depth", "2", "--vit-heads", "2", "--out-dim", "256",
              "--img-size", "32", "--batch-size", "4", "--synthetic", "16", "--num-workers", "0", "--warmup-steps", "2", "--lr", "1e-3",
              "--max-steps", "4", "--streams", "off", "--monitor-every", "0", "--run-dir", str(tmp_path / "run")])
    capsys.readouterr()
    ckpt = sorted((tmp_path / "run").iterdir())[-1] / "checkpoint_final_00000004.pth"
    spec = importlib.util.spec_from_file_location("phase5_monitor", os.path.join(os.path.dirname(cli.__file__), "phase5_monitor.py"))
    mon = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mon
    spec.loader.exec_module(mon)
    seen = {}
    for name, extra in (("off", []), ("on", ["--rollout"])):
        assert mon.main(["--checkpoint", str(ckpt), "--synthetic", "8", "--batch-size", "4", "--out-dir", str(tmp_path / name)] + extra) == 0
        out = capsys.readouterr().out
        d = [l.split("=", 1)[1] for l in out.splitlines() if l.startswith("monitor_dir=")][0]
        seen[name] = (set(os.listdir(d)), json.loads(open(os.path.join(d, "stats.json")).read()), d, out)
    assert seen["off"][0] == {n for n in PARENT_FILES if n in seen["off"][0]} and "stats.json" in seen["off"][0]
    assert set(seen["off"][1]) == PARENT_KEYS | {"sample"} and "Rollout:" not in seen["off"][3]
    assert seen["on"][0] - seen["off"][0] == {"rollout.npy"} | ({"rollout.png"} if "heatmap.png" in seen["off"][0] else set())
    assert set(seen["on"][1]) - set(seen["off"][1]) == {"rollout_patch_mass", "rollout_entropy"} and "Rollout:" in seen["on"][3]
    assert all(seen["on"][1][k] == seen["off"][1][k] for k in seen["off"][1])
    assert np.load(os.path.join(seen["on"][2], "rollout.npy")).shape == (2, 2)
