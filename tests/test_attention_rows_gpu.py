"""dinox_attention_rows on the device: every element against the float64 oracle inside the a-priori bound of
tests/_attention_rows_oracle.py (nothing masked or left out), bit reproducibility, the lse against the attention core's, the model and
inference surfaces, and a training run that the monitor must leave bit-identical (engine and CLI).

The bound tests print their largest err / bound ratio per family and dtype (run with -s); DESIGN.md section 4, "Attention rows", is where
the measured table belongs."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import load_golden

import _attention_rows_oracle as RO
from oracle import attention_bounds as AB

pytestmark = pytest.mark.gpu

DEV = "cuda"
# N: one key, under one wave, the edges of a wave, two blocks' worth of lanes (201: ViT-S/16 at 224; 257: one key past the 256-thread
# stride).  d: 16 and 64 take the 16-byte loads in both dtypes, 88 (ViT-g) is no power of two, 12 takes them in fp32 only, 7 in neither.
NS = (1, 5, 63, 64, 65, 201, 257)
DS = (16, 64, 88, 7, 12)


def query_sets(N):
    return [(0,), (0, N - 1), tuple((3 * i + 1) % N for i in range(7)) + (1 % N,), (N - 1,)]


@pytest.fixture(scope="module")
def dx():
    from dinox import ops
    import zoo.arch as arch
    import dinox._lib as L
    assert L.lib.dinox_device_ok() == 1, L.last_error()
    return ops, arch


def run_case(ops, case, dtype, B, N, heads, d, idx, seed, worst):
    qkv = AB.make_qkv(case, B, N, heads, d, seed=seed, dtype=dtype)
    ref = RO.rows_oracle(qkv, heads, idx)
    probs, lse = ops.attention_rows(qkv.to(DEV), heads, idx, want_lse=True)
    assert probs.shape == (B, heads, len(idx), N) and probs.dtype == torch.float32 and lse.shape == (B, heads, len(idx))
    r = RO.check_rows(probs, lse, ref, f"{case} {dtype} B={B} N={N} heads={heads} d={d} idx={idx}")
    for k, v in r.items():
        worst[k] = max(worst.get(k, 0.0), v)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", AB.FAMILIES)
def test_rows_inside_the_bound_elementwise(dx, case, dtype):
    ops, _ = dx
    worst = {}
    n = 0
    for N in NS:
        for d in DS:
            heads, B = (1, 3) if n % 2 else (3, 1)
            n += 1
            for idx in query_sets(N):
                run_case(ops, case, dtype, B, N, heads, d, idx, 100 + n, worst)
    run_case(ops, case, dtype, 3, 65, 3, 64, (0, 64), 7, worst)               # several images AND several heads
    run_case(ops, case, dtype, 1, 9, 1, 256, (0, 8), 8, worst)                # the largest head size
    print(f"attention_rows {case} {dtype}: largest err / bound  probs {worst['p']:.4f}  row sum {worst['sum']:.4f}  lse {worst['lse']:.4f}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", AB.FAMILIES)
def test_rows_at_vit_l_518_tokens(dx, case, dtype):
    """N = 1374 (518 px at patch 14, 4 registers): six keys per thread, a ragged last stride."""
    ops, _ = dx
    worst = {}
    run_case(ops, case, dtype, 1, 1374, 2, 64, (0, 1373, 700), 21, worst)
    print(f"attention_rows N=1374 {case} {dtype}: largest err / bound  probs {worst['p']:.4f}  row sum {worst['sum']:.4f}  lse {worst['lse']:.4f}")


def test_unaligned_base_takes_the_scalar_path(dx):
    """A packed tensor that starts one element into its allocation is contiguous but not 16-byte aligned."""
    ops, _ = dx
    for dtype in (torch.float32, torch.bfloat16):
        qkv = AB.make_qkv("ramp", 2, 65, 2, 16, seed=4, dtype=dtype)
        buf = torch.empty(qkv.numel() + 1, dtype=dtype, device=DEV)
        view = buf[1:].view(qkv.shape)
        view.copy_(qkv)
        assert view.data_ptr() % 16 != 0 and view.is_contiguous()
        ref = RO.rows_oracle(qkv, 2, (0, 64))
        probs, lse = ops.attention_rows(view, 2, (0, 64), want_lse=True)
        RO.check_rows(probs, lse, ref, f"unaligned {dtype}")
        assert torch.equal(probs, ops.attention_rows(qkv.to(DEV), 2, (0, 64)))       # the two load paths add in the same order


def test_layouts_index_tensors_and_errors(dx):
    ops, _ = dx
    qkv = AB.make_qkv("randn", 2, 33, 3, 16, seed=5, dtype=torch.float32).to(DEV)
    a = ops.attention_rows(qkv, 3, (0, 32))
    assert torch.equal(a, ops.attention_rows(qkv.view(2, 33, 3, 3, 16), 3, torch.tensor([0, 32], device=DEV)))
    assert torch.equal(a, ops.attention_rows(qkv, 3, torch.tensor([0, 32], dtype=torch.int32)))
    assert torch.equal(a[:, :, 1], ops.attention_rows(qkv, 3, [32])[:, :, 0])           # a row does not depend on its neighbours
    assert isinstance(a, torch.Tensor) and not a.requires_grad
    assert not ops.attention_rows(qkv.clone().requires_grad_(), 3, (0,)).requires_grad   # no gradient is defined
    with pytest.raises(ValueError, match="outside"):
        ops.attention_rows(qkv, 3, (33,))
    with pytest.raises(ValueError, match="query rows"):
        ops.attention_rows(qkv, 3, list(range(9)))
    with pytest.raises(ValueError, match="device"):
        ops.attention_rows(qkv.cpu(), 3, (0,))
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_bit_reproducible(dx, dtype):
    ops, _ = dx
    qkv = AB.make_qkv("randn", 3, 257, 3, 64, seed=9, dtype=dtype).to(DEV)
    idx = (0, 256, 5, 5)
    p1, l1 = ops.attention_rows(qkv, 3, idx, want_lse=True)
    p2, l2 = ops.attention_rows(qkv, 3, idx, want_lse=True)
    assert torch.equal(p1, p2) and torch.equal(l1, l2)
    assert torch.equal(p1[:, :, 2], p1[:, :, 3])                                          # a repeated index gives the same row


@pytest.mark.parametrize("dtype,N,d", [(torch.bfloat16, 201, 64), (torch.bfloat16, 65, 16), (torch.float32, 201, 64), (torch.float32, 63, 88)],
                         ids=["bf16-mfma", "bf16-d16", "fp32-201", "fp32-d88"])
def test_lse_agrees_with_the_attention_core(dx, dtype, N, d):
    """ops.attention_fwd keeps lse for every row: at the query rows it must agree with attention_rows within the SUM of the two a-priori
    lse bounds (each kernel is within its own bound of float64)."""
    ops, _ = dx
    B, heads = 2, 3
    idx = (0, N - 1, N // 2)
    for case in ("randn", "offset", "lastkey"):
        qkv = AB.make_qkv(case, B, N, heads, d, seed=13, dtype=dtype)
        ref = RO.rows_oracle(qkv, heads, idx)
        fb = AB.forward_bounds(qkv, heads, fp32=dtype == torch.float32)
        _, lse_core = ops.attention_fwd(qkv.to(DEV), heads)
        _, lse_rows = ops.attention_rows(qkv.to(DEV), heads, idx, want_lse=True)
        tol = ref["lse_bound"] + fb["lse_bound"][:, :, list(idx)]
        diff = (lse_core[:, :, list(idx)].double().cpu() - lse_rows.double().cpu()).abs()
        assert bool((diff <= tol).all()), f"{case}: lse differs by {float(diff.max()):.3e}, tolerance {float(tol.min()):.3e}"


# ------------------------------------------------------------------------------------------ model surface
def _tiny(arch, **kw):
    cfg = dict(img_size=56, patch=14, dim=64, depth=2, heads=2, num_registers=2)
    cfg.update(kw)
    return arch.PatchViT(**cfg)


@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "bf16"])
def test_last_attention_feats_are_the_forward_bit_for_bit(dx, amp):
    ops, arch = dx
    torch.manual_seed(0)
    chained = _tiny(arch, scale_aware=True).to(DEV).eval()
    ckpt = _tiny(arch, scale_aware=True, use_grad_checkpoint=True).to(DEV).train()        # train mode: the per-block (unchained) path
    ckpt.load_state_dict(chained.state_dict())
    g = torch.Generator().manual_seed(1)
    x = torch.randn(3, 3, 56, 56, generator=g).to(DEV)
    sp = (torch.rand(3, 3, generator=g) + 0.5).to(DEV)
    seen = {}
    for name, model in (("chained", chained), ("checkpoint", ckpt)):
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            with torch.no_grad():
                want = model(x, sp)
            feats, probs = model.last_attention(x, sp, query_tokens=(0, 17, 18))
            f0, p0 = model.last_attention(x, sp, query_tokens=(0,), layer=0)
        assert torch.equal(feats, want) and torch.equal(f0, want) and not feats.requires_grad
        assert probs.shape == (3, 2, 3, 19) and probs.dtype == torch.float32 and p0.shape == (3, 2, 1, 19)
        assert bool(torch.isfinite(probs).all()) and bool((probs >= 0).all())
        assert float((probs.double().sum(-1) - 1).abs().max()) <= 19 * 2.0 ** -23 + 1e-4
        assert not torch.equal(p0[:, :, 0], probs[:, :, 0])                                # another layer, another map
        seen[name] = (probs, p0)
        assert model.training == (name == "checkpoint")                                   # the mode is left as it was
    tol = 2e-2 if amp else 1e-4                                                           # two launch sequences of one arithmetic
    for a, b in zip(seen["chained"], seen["checkpoint"]):
        assert float((a - b).abs().max()) <= tol


def test_last_attention_rows_are_the_softmax_of_the_blocks_qkv(dx):
    """The qkv product the rows are read from is what the block's own qkv module gives on the block's norm1 output: hooked, then the
    float64 oracle on it."""
    ops, arch = dx
    torch.manual_seed(3)
    model = _tiny(arch).to(DEV).eval()
    x = torch.randn(2, 3, 56, 56, generator=torch.Generator().manual_seed(4)).to(DEV)
    for layer in (0, 1, -1):
        blk = model.blocks[layer]
        got = []
        h = blk.attn.qkv.register_forward_hook(lambda m, i, o: got.append(o.detach()))
        try:
            _, probs = model.last_attention(x, query_tokens=(0, 18), layer=layer)
        finally:
            h.remove()
        assert len(got) == 1 and got[0].shape == (2, 19, 192)
        ref = RO.rows_oracle(got[0].cpu(), 2, (0, 18))
        RO.check_rows(probs, None, ref, f"layer {layer}")
        assert all(len(b.attn.qkv._forward_hooks) == 0 for b in model.blocks)


def test_golden_model_heatmap_and_stats(dx):
    """The reference's make_attention_heatmap and embedding statistics on its own tiny model (monitor_tiny.npz), at the project's
    1e-3 fp32 bar (the heatmap lives in [0, 1]: 1e-3 of its range)."""
    ops, arch = dx
    from dinox.monitor import embedding_stats, patch_norm_heatmap
    g = load_golden("monitor_tiny.npz")
    model = arch.DinoStudentTeacher(_tiny(arch), out_dim=32)
    model.load_state_dict({k[len("state."):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("state.")}, strict=True)
    model = model.to(DEV).eval()
    feats, probs = model.backbone.last_attention(torch.from_numpy(g["batch"]).to(DEV))
    want = torch.from_numpy(g["feats"])
    assert float((feats.cpu() - want).abs().max()) <= 1e-3 * float(want.abs().max())
    heat = patch_norm_heatmap(feats, 16).cpu().numpy()
    np.testing.assert_allclose(heat, g["heatmap"], rtol=1e-3, atol=1e-3)
    st = embedding_stats(feats[:, 0])
    for k in ("embedding_std_mean", "embedding_norm_mean"):
        assert abs(st[k] - float(g[k])) <= 1e-3 * abs(float(g[k])), (k, st[k], float(g[k]))
    assert probs.shape == (8, 2, 1, 19)


def test_attention_map(dx):
    ops, arch = dx
    from zoo.encode import attention_map, encode
    torch.manual_seed(0)
    vit = arch.PatchViT(img_size=32, patch=16, dim=64, depth=2, heads=4).to(DEV).eval()
    img = np.random.default_rng(0).uniform(-1000, 1000, size=(48, 40)).astype(np.float32)
    m = attention_map(vit, img, (0.7, 0.7), 2.5)
    assert m.shape == (4, 2, 2) and m.dtype == torch.float32 and m.device.type == "cpu"
    assert bool(torch.isfinite(m).all()) and bool((m >= 0).all()) and bool((m.sum((-1, -2)) <= 1.0).all()) and bool((m.sum((-1, -2)) > 0).all())
    assert torch.equal(m, attention_map(vit, img))                                        # not scale-aware: spacing is not used
    assert m.shape == attention_map(vit, img, preprocess="auto", layer=0).shape
    with pytest.raises(ValueError, match="Unknown input_format"):
        attention_map(vit, img, input_format="nope")
    with pytest.raises(ValueError, match="Unsupported image shape"):
        attention_map(vit, np.zeros((2, 3, 4, 5), np.float32))
    assert encode(vit, img).shape == (1, 1, 64)                                           # the existing surface is untouched


# ------------------------------------------------------------------------------------------ training is untouched
@pytest.mark.parametrize("graph,amp", [(False, False), (True, False), (True, True)], ids=["eager", "graph", "graph-bf16"])
def test_monitor_leaves_the_training_state_bit_identical(dx, tmp_path, graph, amp):
    """Four steps with run_monitor after steps 2 and 4 against four steps without.  With use_graph the first call falls between the
    last eager step and the capture, the second between two replays; in bf16 the 14-pixel patch weight has a cached padded image,
    which a capture must not inherit from the monitor."""
    ops, arch = dx
    from dinox.engine import StepHyperParams, TrainEngine
    from dinox.monitor import run_monitor
    kw = dict(img_size=56, patch=14, dim=64, depth=2, heads=2, num_registers=2, scale_aware=True)
    gen = torch.Generator().manual_seed(6)
    batches = [(torch.randn(8, 3, 56, 56, generator=gen).to(DEV), (torch.rand(8, 3, generator=gen) + 0.5).to(DEV)) for _ in range(4)]

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
                    out.append(run_monitor(s_.backbone, b, sp, tmp_path / f"mon_{int(graph)}", i + 1))
        torch.cuda.synchronize()
        assert (eng._graph is not None) == graph
        return [t.clone() for t in (eng.flat_p, eng.flat_t, eng.center, eng.adam_m, eng.adam_v)], out

    plain, _ = run(False)
    watched, stats = run(True)
    for name, a, b in zip(("flat_p", "flat_t", "center", "adam_m", "adam_v"), plain, watched):
        assert torch.equal(a, b), name
    assert [s["step"] for s in stats] == [2, 4] and all(np.isfinite(s["embedding_std_mean"]) and s["batch"] == 8 for s in stats)
    d = tmp_path / f"mon_{int(graph)}" / "step_00000004"
    assert np.load(d / "attention.npy").shape == (2, 4, 4) and np.load(d / "heatmap.npy").shape == (4, 4)
    assert np.array_equal(np.load(d / "input.npy"), batches[3][0][0, 1].cpu().numpy())


def test_cli_writes_the_monitor_and_trains_the_same(dx, cli, tmp_path, capsys):
    common = ["--config", "custom", "--vit-patch", "16", "--vit-dim", "64", "--vit-depth", "2", "--vit-heads", "2", "--out-dim", "256",
              "--img-size", "32", "--batch-size", "4", "--synthetic", "16", "--num-workers", "0", "--warmup-steps", "2", "--lr", "1e-3",
              "--max-steps", "4", "--streams", "off"]
    cli.main(common + ["--monitor-every", "2", "--run-dir", str(tmp_path / "on")])
    out = capsys.readouterr().out
    assert out.count("monitor_saved=") == 2
    cli.main(common + ["--monitor-every", "0", "--run-dir", str(tmp_path / "off")])
    assert "monitor_saved=" not in capsys.readouterr().out
    run_on, run_off = sorted((tmp_path / "on").iterdir())[-1], sorted((tmp_path / "off").iterdir())[-1]
    assert sorted(p.name for p in (run_on / "monitor").iterdir()) == ["step_00000002", "step_00000004"] and not (run_off / "monitor").exists()
    for step in (2, 4):
        d = run_on / "monitor" / f"step_{step:08d}"
        assert {"heatmap.npy", "attention.npy", "input.npy", "stats.json"} <= {p.name for p in d.iterdir()}
        st = json.loads((d / "stats.json").read_text())
        assert st["step"] == step and st["batch"] == 8 and len(st["attention_entropy"]) == 2
        assert np.isfinite(st["embedding_std_mean"]) and np.isfinite(st["embedding_norm_mean"])
        assert all(0.0 <= e <= st["attention_entropy_max"] + 1e-5 for e in st["attention_entropy"])
        assert np.load(d / "attention.npy").shape == (2, 2, 2) and np.load(d / "heatmap.npy").shape == (2, 2) and np.load(d / "input.npy").shape == (32, 32)
    a = torch.load(run_on / "checkpoint_final_00000004.pth", map_location="cpu", weights_only=False)
    b = torch.load(run_off / "checkpoint_final_00000004.pth", map_location="cpu", weights_only=False)
    assert set(a["student"]) == set(b["student"]) and all(torch.equal(a["student"][k], b["student"][k]) for k in a["student"])
    assert all(torch.equal(a["teacher"][k], b["teacher"][k]) for k in a["teacher"])

    # the monitor script on that checkpoint
    import importlib.util
    import sys
    spec = importlib.util.spec_from_file_location("phase5_monitor", os.path.join(os.path.dirname(cli.__file__), "phase5_monitor.py"))
    mon = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mon
    spec.loader.exec_module(mon)
    assert mon.main(["--checkpoint", str(run_on / "checkpoint_final_00000004.pth"), "--synthetic", "8", "--batch-size", "4",
                     "--out-dir", str(tmp_path / "mon")]) == 0
    out = capsys.readouterr().out
    d = [l.split("=", 1)[1] for l in out.splitlines() if l.startswith("monitor_dir=")][0]
    st = json.loads(open(os.path.join(d, "stats.json")).read())
    assert {"step", "embedding_std_mean", "embedding_norm_mean", "sample", "attention_entropy"} <= set(st) and st["step"] == 4 and st["batch"] == 5
    assert np.load(os.path.join(d, "attention.npy")).shape == (2, 2, 2) and np.load(os.path.join(d, "heatmap.npy")).shape == (2, 2)
