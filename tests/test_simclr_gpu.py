"""SimCLR objective on the device: the NT-Xent kernels against the reference fixture and the float64 oracle, the engine's
``loss_type="simclr"`` step against three steps of the reference loop (tests/golden/simclr_step_tiny.npz), accumulation, hipGraph
replay and the CLI.  These tests pin the reference fixtures at the project's parity bar; the element-wise judge of each NT-Xent
kernel (a-priori fp32 bounds against float64, hostile S) is tests/test_ntxent_bounds_gpu.py."""
import json

import numpy as np
import pytest
import torch

from conftest import load_golden, sub, t

import _ntxent_oracle as NX

pytestmark = pytest.mark.gpu

DEV = "cuda"
CASES = ["b3", "b33", "b130", "adv"]          # 2B = 6 (under one wavefront, odd D), 66 (crosses 64 lanes, D % 4 != 0),
#                                               260 (more than one 256-thread stride), 16 adversarial rows


@pytest.fixture(scope="module")
def dx():
    from dinox import ops
    import zoo.arch as arch
    import dinox._lib as L
    assert L.lib.dinox_device_ok() == 1, L.last_error()
    return ops, arch


@pytest.fixture(scope="module")
def gold():
    return load_golden("simclr_loss.npz")


@pytest.fixture(scope="module")
def oracle(gold):
    """float64 oracle loss and dz per case, computed once."""
    return {tag: NX.ntxent(np.concatenate([gold[f"{tag}_z1"], gold[f"{tag}_z2"]], 0), 0.1) for tag in CASES}


def row_err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = np.abs(want).max(1)
    err = np.abs(got - want).max(1)
    zero = scale == 0
    return float((err[~zero] / scale[~zero]).max()), float(err[zero].max()) if zero.any() else 0.0


@pytest.mark.parametrize("tag", CASES)
def test_ntxent_kernels_match_reference_and_oracle(dx, gold, oracle, tag):
    """The project's parity bar: loss rel 1e-3, every gradient row within 1e-3 of that row's max-abs in the reference; all finite."""
    ops, _ = dx
    z = torch.from_numpy(np.concatenate([gold[f"{tag}_z1"], gold[f"{tag}_z2"]], 0)).to(DEV)
    loss, saved = ops.ntxent_fwd(z, 0.1)
    dz = ops.ntxent_bwd(saved, 1.0)
    loss, dz = float(loss), dz.cpu().numpy()
    assert np.isfinite(loss) and np.isfinite(dz).all()
    ref_dz = np.concatenate([gold[f"{tag}_dz1"], gold[f"{tag}_dz2"]], 0)
    o_loss, o_dz = oracle[tag]
    for name, want_loss, want_dz in (("reference", float(gold[f"{tag}_loss"]), ref_dz), ("oracle", o_loss, o_dz)):
        e_row, e_zero = row_err(dz, want_dz)
        print(f"{tag} vs {name}: loss rel err {abs(loss - want_loss) / abs(want_loss):.2e}, worst gradient row {e_row:.2e}")
        assert abs(loss - want_loss) <= 1e-3 * abs(want_loss)
        assert e_row <= 1e-3 and e_zero == 0.0
    # an upstream factor scales the gradient and nothing else
    dz3 = ops.ntxent_bwd(saved, 0.25).cpu().numpy()
    assert row_err(dz3, 0.25 * o_dz)[0] <= 1e-3


def test_ntxent_second_ragged_chunk_of_the_row_sum(dx):
    """B = 513, D = 32: M = 1026 rows, so the row-loss sum (ntxent_sum_kernel, 1024 rows of LDS per pass) takes a second pass of
    2 rows -- no fixture is that large, the input is drawn here from a fixed seed.  Loss and gradient against the float64 oracle at the
    bar of the cases above, through the square path (the mean form: divisor M) and, force_rect=True, the rectangular one (the sum
    form: divisor 1, the host divides)."""
    ops, _ = dx
    z = torch.randn(1026, 32, generator=torch.Generator().manual_seed(513))
    o_loss, o_dz = NX.ntxent(z.numpy(), 0.1)
    for rect in (False, True):
        loss, saved = ops.ntxent_fwd(z.to(DEV), 0.1, force_rect=rect)
        dz = ops.ntxent_bwd(saved, 1.0).cpu().numpy()
        loss = float(loss)
        assert np.isfinite(loss) and np.isfinite(dz).all()
        e_row, e_zero = row_err(dz, o_dz)
        print(f"M=1026 {'rect' if rect else 'square'}: loss rel err {abs(loss - o_loss) / abs(o_loss):.2e}, worst gradient row {e_row:.2e}")
        assert abs(loss - o_loss) <= 1e-3 * abs(o_loss)
        assert e_row <= 1e-3 and e_zero == 0.0


@pytest.mark.parametrize("tag", ["b33", "b130", "adv"])
def test_ntxent_is_bit_reproducible(dx, gold, tag):
    ops, _ = dx
    z = torch.from_numpy(np.concatenate([gold[f"{tag}_z1"], gold[f"{tag}_z2"]], 0)).to(DEV)
    runs = []
    for _ in range(2):
        loss, saved = ops.ntxent_fwd(z.clone(), 0.1)
        runs.append((loss.clone(), ops.ntxent_bwd(saved, 1.0)))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_autograd_path_equals_manual_path_bitwise(dx, gold):
    ops, _ = dx
    z1 = torch.from_numpy(gold["b33_z1"]).to(DEV).requires_grad_(True)
    z2 = torch.from_numpy(gold["b33_z2"]).to(DEV).requires_grad_(True)
    loss = ops.simclr_loss(z1, z2, 0.1)
    g1, g2 = torch.autograd.grad(loss, [z1, z2])
    m_loss, saved = ops.ntxent_fwd(torch.cat([z1.detach(), z2.detach()], 0), 0.1)
    dz = ops.ntxent_bwd(saved, 1.0)
    assert loss.dim() == 0 and torch.equal(loss.detach().reshape(1), m_loss)
    assert torch.equal(g1, dz[:33]) and torch.equal(g2, dz[33:])


def test_error_paths_launch_nothing(dx):
    ops, _ = dx
    import dinox._lib as L
    with pytest.raises(ValueError, match="2B"):
        ops.ntxent_fwd(torch.randn(5, 8, device=DEV))
    with pytest.raises(ValueError, match="2B"):
        ops.ntxent_fwd(torch.randn(8, device=DEV))
    with pytest.raises(ValueError, match=r"\[B, D\]"):
        ops.simclr_loss(torch.randn(3, 8, device=DEV), torch.randn(4, 8, device=DEV))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ntxent_fwd(torch.randn(4, 8))
    # the C entry points themselves: odd M on real device buffers returns EINVAL and leaves the outputs untouched
    S = torch.randn(5, 5, device=DEV)
    out = torch.full((12,), -7.0, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    assert L.lib.dinox_ntxent_rows(S.data_ptr(), 5, 5, 10.0, out.data_ptr(), out.data_ptr() + 20, out.data_ptr() + 40, st) == -1
    assert "M=5" in L.last_error()
    W = torch.full((5, 5), -7.0, device=DEV)
    assert L.lib.dinox_ntxent_coeff(S.data_ptr(), 5, out.data_ptr(), 5, 10.0, 1.0, W.data_ptr(), 5, st) == -1
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((W == -7.0).all())


# ------------------------------------------------------------------------------------------ the engine
def _cfg(arr):
    img, patch, dim, depth, heads, regs, sa, out = [int(v) for v in arr]
    return dict(img_size=img, patch=patch, dim=dim, depth=depth, heads=heads, num_registers=regs, scale_aware=bool(sa)), out


def _tiny_engine(arch, g, accum=1, **kw):
    from dinox.engine import StepHyperParams, TrainEngine
    cfg, out_dim = _cfg(g["cfg"])
    lr, min_lr, warm, max_steps, wd, temp = [float(v) for v in g["hp"]]
    hp = StepHyperParams(lr=lr, min_lr=min_lr, warmup_steps=int(warm), max_steps=int(max_steps), weight_decay=wd, loss_type="simclr",
                         simclr_temp=temp)
    init = {k: v.float() for k, v in sub(g, "init").items()}
    student = arch.DinoStudentTeacher(arch.PatchViT(**cfg), out_dim)
    teacher = arch.DinoStudentTeacher(arch.PatchViT(**cfg), out_dim)
    student.load_state_dict(init)
    teacher.load_state_dict(init)
    return TrainEngine(student.to(DEV), teacher.to(DEV), out_dim, hp, accumulation_steps=accum, **kw), student, teacher, init


def _batch(g, step):
    return t(g[f"batch{step}"]).float().to(DEV), t(g[f"spacing{step}"]).to(DEV)


@pytest.mark.parametrize("top", ["manual", "autograd"])
def test_engine_three_steps_match_the_reference(dx, monkeypatch, top):
    """fp32 mode against three steps of the reference loop with loss_type="simclr": scalars per step, every gradient of step 0, the
    weights after step 3 -- and the teacher and the centre exactly as initialised.  Both tops: the head and the loss written out by hand
    (the default) and through the per-op autograd nodes (DINOX_AUTOGRAD_TOP=1, read when the engine is built)."""
    _, arch = dx
    if top == "autograd":
        monkeypatch.setenv("DINOX_AUTOGRAD_TOP", "1")
    else:
        monkeypatch.delenv("DINOX_AUTOGRAD_TOP", raising=False)
    g = load_golden("simclr_step_tiny.npz")
    eng, student, teacher, init = _tiny_engine(arch, g)
    assert eng.manual_top == (top == "manual")
    names = [str(n) for n in g["param_order"]]
    for step in range(3):
        eng.step(*_batch(g, step))
        r = eng.scalars()
        print(f"step {step}: loss {r['loss']:.6f} vs {float(g['losses'][step]):.6f}, grad-norm {r['grad_norm']:.5f} vs "
              f"{float(g['grad_norms'][step]):.5f}")
        assert r["loss"] == pytest.approx(float(g["losses"][step]), rel=1e-3)
        assert r["simclr"] == r["loss"] and r["dino"] == 0.0 and r["gram"] == 0.0 and r["koleo"] == 0.0
        assert r["grad_norm"] == pytest.approx(float(g["grad_norms"][step]), rel=1e-3)
        assert r["lr"] == pytest.approx(float(g["lrs"][step]), rel=1e-12)
        if step == 0:
            worst = (0.0, "")
            for n, p in student.named_parameters():
                want = t(g[f"grad0/{n}"]).double()
                err = float((p.grad.cpu().double() - want).abs().max())
                bound = 1e-3 * float(want.abs().max()) + 1e-7
                worst = max(worst, (err / bound, n))
                assert err <= bound, (n, err, bound)
            print(f"step 0 gradients: worst tensor {worst[1]} at {worst[0]:.3f} of its bound")
    assert [n for n, _ in student.named_parameters()] == names
    share = float(g["small_grad_share"])
    assert share <= 0.10
    lr_sum = float(sum(float(v) for v in g["lrs"][:3]))
    have, want_sd = student.state_dict(), sub(g, "student3")
    n_tight = n_bad = 0
    for k, v in want_sd.items():
        d = (have[k].cpu().double() - v.double()).abs()
        m = torch.zeros_like(v, dtype=torch.bool)
        for step in range(3):
            m |= t(g[f"grad{step}/{k}"]).abs() < 1e-6        # Adam turns a numerically-zero gradient into a +-lr move of round-off sign
        if m.any():
            assert float(d[m].max()) <= 2.1 * lr_sum, (k, float(d[m].max()))
        tight = d[~m]
        n_tight += tight.numel()
        n_bad += int((tight > 1e-3 * v.double().abs()[~m] + 2e-5).sum())
    print(f"weights after step 3: {n_bad} of {n_tight} elements outside 1e-3 |v| + 2e-5")
    assert n_bad <= 1e-4 * n_tight, (n_bad, n_tight)
    tsd = teacher.state_dict()
    for k, v in init.items():
        assert torch.equal(tsd[k].cpu(), v), f"teacher {k} moved"
    assert bool((eng.center == 0).all())


def test_engine_accumulation_averages_the_micro_batch_gradients(dx):
    """accumulation_steps = 2: after two micro-batches the gradient arena holds (g(batch 0) + g(batch 1)) / 2, both at the initial
    weights (no optimiser step in between).  Reference: the engine itself at accumulation 1, one fresh engine per batch -- its
    arena still holds the step's gradient after the optimiser ran.  Bound per tensor: 1e-5 of its max-abs (the factor 1/2 is exact in
    fp32; what differs is the order of a handful of fp32 additions, ~1e-7 each)."""
    _, arch = dx
    g = load_golden("simclr_step_tiny.npz")
    singles = []
    for step in range(2):
        e1, _, _, _ = _tiny_engine(arch, g)
        e1.step(*_batch(g, step))
        singles.append((e1.flat_g.clone(), float(e1.last["loss"])))
    e2, student, _, _ = _tiny_engine(arch, g, accum=2)
    p0 = e2.flat_p.clone()
    e2.step(*_batch(g, 0))
    assert torch.equal(e2.flat_p, p0) and e2.opt_steps == 0 and float(e2.last["grad_norm_sq"]) == 0.0
    assert float(e2.last["loss"]) == singles[0][1]
    e2.step(*_batch(g, 1))
    assert e2.opt_steps == 1 and not torch.equal(e2.flat_p, p0)
    assert float(e2.last["loss"]) == singles[1][1]                 # the logged loss is the micro-batch's own, undivided
    want = 0.5 * (singles[0][0].double() + singles[1][0].double())
    worst = 0.0
    for (n, p), off in zip(student.named_parameters(), e2.offsets):
        w = want[off:off + p.numel()]
        err = float((e2.flat_g[off:off + p.numel()].double() - w).abs().max())
        worst = max(worst, err / float(w.abs().max()))
        assert err <= 1e-5 * float(w.abs().max()), (n, err, float(w.abs().max()))
    print(f"accumulated gradient: worst tensor at {worst:.2e} of its max-abs")
    assert float(e2.last["grad_norm_sq"]) == pytest.approx(float((want * want).sum()), rel=1e-4)


def test_engine_grad_checkpoint_and_bf16_mode(dx):
    """--grad-checkpoint recomputes the blocks in backward: same step to round-off.  bf16 throughput mode: the step runs, stays finite
    and close to the fp32 step (the NT-Xent head itself is fp32 in both modes)."""
    _, arch = dx
    from dinox.engine import StepHyperParams, TrainEngine
    g = load_golden("simclr_step_tiny.npz")
    cfg, out_dim = _cfg(g["cfg"])
    init = {k: v.float() for k, v in sub(g, "init").items()}

    def run(ckpt, amp):
        s_ = arch.DinoStudentTeacher(arch.PatchViT(use_grad_checkpoint=ckpt, **cfg), out_dim)
        t_ = arch.DinoStudentTeacher(arch.PatchViT(**cfg), out_dim)
        s_.load_state_dict(init)
        t_.load_state_dict(init)
        eng = TrainEngine(s_.to(DEV), t_.to(DEV), out_dim, StepHyperParams(lr=1e-3, warmup_steps=2, max_steps=10, loss_type="simclr"), amp_dtype=amp)
        eng.step(*_batch(g, 0))
        return eng.scalars(), eng.flat_g.clone()

    (s0, g0), (s1, g1), (s2, g2) = run(False, None), run(True, None), run(False, torch.bfloat16)
    assert s1["loss"] == pytest.approx(s0["loss"], rel=1e-6) and s1["grad_norm"] == pytest.approx(s0["grad_norm"], rel=1e-5)
    assert float((g1 - g0).abs().max()) <= 1e-5 * float(g0.abs().max())
    assert np.isfinite(s2["loss"]) and bool(torch.isfinite(g2).all())
    assert s2["loss"] == pytest.approx(s0["loss"], rel=5e-2) and s2["grad_norm"] == pytest.approx(s0["grad_norm"], rel=0.1)


def test_engine_rejects_what_simclr_does_not_cover(dx):
    _, arch = dx
    from dinox.engine import StepHyperParams
    g = load_golden("simclr_step_tiny.npz")
    eng, _, _, _ = _tiny_engine(arch, g)
    batch, sp = _batch(g, 0)
    with pytest.raises(ValueError, match="local crops"):
        eng.step(batch, sp, torch.randn(8, 3, 14, 14, device=DEV), sp)
    assert eng.step_count == 0
    with pytest.raises(ValueError, match="loss_type"):
        from dinox.engine import TrainEngine
        TrainEngine(eng.student, eng.teacher, 64, StepHyperParams(loss_type="mae"))


def test_graph_replay_equals_eager_bitwise(dx):
    """use_graph=True: two eager steps, capture, replay -- four steps leave the student arena bit-identical to four eager steps
    (every reduction of the step has a fixed order), the teacher arena untouched."""
    _, arch = dx
    g = load_golden("simclr_step_tiny.npz")
    batches = [_batch(g, s % 3) for s in range(4)]
    batches[3] = (batches[3][0].flip(0).contiguous(), batches[3][1].flip(0).contiguous())      # a fourth, different batch

    def run(graph):
        eng, _, _, _ = _tiny_engine(arch, g, use_graph=graph)
        t0 = eng.flat_t.clone()
        losses = []
        for b, s in batches:
            eng.step(b, s)
            losses.append(eng.scalars()["loss"])
        assert (eng._graph is not None) == graph and eng.step_count == 4 and eng.opt_steps == 4
        assert torch.equal(eng.flat_t, t0) and bool((eng.center == 0).all())
        return losses, eng.flat_p.clone(), eng.adam_m.clone(), eng.adam_v.clone()

    le, pe, me, ve = run(False)
    lg, pg, mg, vg = run(True)
    assert lg == le and len(set(lg)) == 4
    assert torch.equal(pg, pe) and torch.equal(mg, me) and torch.equal(vg, ve)


def test_dino_step_keeps_its_phases_and_simclr_drops_the_teacher(dx, monkeypatch):
    """What can be observed of the launch sequence from the host: a dino step still passes its seven phase marks in order and moves the
    teacher and the centre; a simclr step on the same model has no teacher phase and launches fewer products; a mae step (a tiny
    encoder under a tiny decoder, no teacher at all) passes the same six marks as simclr and leaves the centre alone."""
    ops, arch = dx
    from dinox.engine import StepHyperParams, TrainEngine
    from dinox.mae import MaeModel
    monkeypatch.delenv("DINOX_SIDE_STREAM", raising=False)     # (a CLI run earlier in the process sets it: the forked teacher chain has no marks)
    g = load_golden("simclr_step_tiny.npz")
    cfg, out_dim = _cfg(g["cfg"])
    init = {k: v.float() for k, v in sub(g, "init").items()}
    seen = {}
    for loss_type in ("dino", "simclr", "mae"):
        if loss_type == "mae":                                 # (the shapes of tests/golden/mae_step_tiny.npz)
            torch.manual_seed(4)
            s_ = MaeModel(arch.PatchViT(img_size=32, patch=8, dim=32, depth=2, heads=2, num_registers=2, scale_aware=True), decoder_dim=32,
                          decoder_depth=2, decoder_heads=4).to(DEV)
            t_, inputs = None, (torch.randn(6, 3, 32, 32, device=DEV), None)
        else:
            s_ = arch.DinoStudentTeacher(arch.PatchViT(**cfg), out_dim)
            t_ = arch.DinoStudentTeacher(arch.PatchViT(**cfg), out_dim)
            s_.load_state_dict(init)
            t_.load_state_dict(init)
            s_, t_, inputs = s_.to(DEV), t_.to(DEV), _batch(g, 0)
        eng = TrainEngine(s_, t_, out_dim, StepHyperParams(lr=1e-3, warmup_steps=2, max_steps=10, ema=0.9, loss_type=loss_type))
        t0 = None if eng.flat_t is None else eng.flat_t.clone()
        eng.marks, ops.TRACE_KERNELS = [], []
        try:
            eng.step(*inputs)
        finally:
            products, ops.TRACE_KERNELS = ops.TRACE_KERNELS, None
        seen[loss_type] = ([n for n, _ in eng.marks], len(products), t0 is not None and not torch.equal(eng.flat_t, t0),
                           bool((eng.center != 0).any()), set(eng.scalars()))
    assert seen["dino"][0] == ["start", "fwd_student", "fwd_teacher", "loss", "bwd", "comm_exposed", "optimiser_tail"]
    assert seen["dino"][2] and seen["dino"][3]
    assert seen["simclr"][0] == ["start", "fwd_student", "loss", "bwd", "comm_exposed", "optimiser_tail"]
    assert not seen["simclr"][2] and not seen["simclr"][3] and seen["simclr"][1] < seen["dino"][1]
    assert seen["mae"][0] == ["start", "fwd_student", "loss", "bwd", "comm_exposed", "optimiser_tail"]
    assert not seen["mae"][2] and not seen["mae"][3]
    # a dino engine reports exactly the scalars it always did (callers iterate over them); simclr and mae add their own
    assert seen["dino"][4] == {"loss", "dino", "gram", "koleo", "grad_norm", "lr"} and seen["simclr"][4] == seen["dino"][4] | {"simclr"}
    assert seen["mae"][4] == seen["dino"][4] | {"mae"}


# ------------------------------------------------------------------------------------------ CLI end to end
def test_cli_simclr_trains_checkpoints_and_resumes(dx, cli, tmp_path, capsys):
    common = ["--config", "vit-tiny", "--vit-patch", "16", "--vit-dim", "64", "--vit-depth", "2", "--vit-heads", "2", "--out-dim", "256",
              "--img-size", "32", "--batch-size", "8", "--scale-aware", "--synthetic", "64", "--num-workers", "0", "--warmup-steps", "2",
              "--lr", "1e-3", "--ckpt-every", "3", "--loss-type", "simclr", "--run-dir", str(tmp_path / "runs")]
    log1 = tmp_path / "a.jsonl"
    cli.main(common + ["--max-steps", "3", "--log-json", str(log1)])
    out = capsys.readouterr().out
    assert "checkpoint_saved=" in out and "final_checkpoint=" in out
    lines = [json.loads(l) for l in log1.read_text().splitlines()]
    assert [l["step"] for l in lines] == [0, 1, 2] and all(set(l) == {"step", "loss", "lr"} and np.isfinite(l["loss"]) for l in lines)
    assert all(0.0 < l["loss"] <= np.log(15) + 20.0 for l in lines)  # NT-Xent's range at 2B = 16, tau = 0.1: (0, log(2B - 1) + 2 / tau]
    run = sorted((tmp_path / "runs").iterdir())[-1]
    assert sorted(p.name for p in run.glob("*.pth")) == ["checkpoint_00000003.pth", "checkpoint_final_00000003.pth"]
    assert json.loads((run / "config.json").read_text())["loss_type"] == "simclr"
    payload = torch.load(run / "checkpoint_00000003.pth", map_location="cpu", weights_only=False)
    assert {"step", "student", "teacher", "opt", "scaler", "dino_loss", "rng", "config"} <= set(payload)
    assert bool((payload["dino_loss"]["center"] == 0).all())
    moved = [k for k in payload["student"] if not torch.equal(payload["student"][k], payload["teacher"][k])]
    assert len(moved) > 0.9 * len(payload["student"])                # the student trained; the teacher is the initial copy
    log2 = tmp_path / "b.jsonl"
    cli.main(common + ["--max-steps", "4", "--log-json", str(log2), "--resume", "auto"])
    out = capsys.readouterr().out
    assert "resumed_from_step=3" in out
    cont = [json.loads(l) for l in log2.read_text().splitlines()]
    assert [l["step"] for l in cont] == [3] and np.isfinite(cont[0]["loss"])
    after = torch.load(sorted(run.glob("checkpoint_final_*.pth"))[-1], map_location="cpu", weights_only=False)
    assert after["step"] == 4 and all(torch.equal(after["teacher"][k], payload["teacher"][k]) for k in payload["teacher"])


def test_cli_mae_still_exits_with_its_message(dx, cli):
    with pytest.raises(SystemExit, match="mae is not wired"):
        cli.main(["--loss-type", "mae", "--synthetic", "8"])
