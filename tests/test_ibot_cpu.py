"""CPU checks of the iBOT masked-patch objective: the host mask generator, the float64 oracle against a literal autograd statement,
the fp32 evaluation of the oracle inside its own bounds, the parser's and the engine's refusals, the model's initial weights, and the
host-side argument checks of the new entry points.  No kernel is launched here."""
import random

import numpy as np
import pytest
import torch

import _ibot_oracle as IO


# ------------------------------------------------------------------------------------------ masks
@pytest.mark.parametrize("grid,ratio", [(2, (0.1, 0.5)), (4, (0.1, 0.5)), (14, (0.1, 0.5)), (14, (0.9, 1.0)), (7, (0.3, 0.3))])
def test_mask_counts_order_range_and_weights(grid, ratio):
    from dinox.ibot import MaskGenerator
    P, V, R = grid * grid, 12, 4
    g = MaskGenerator(3, grid, registers=R, mask_prob=0.7, ratio=ratio)
    for _ in range(6):
        m = g.draw(V)
        idx, w, tok = m.triple()
        assert idx.dtype == np.int32 and w.dtype == np.float32 and tok.dtype == np.int32 and len(idx) == len(w) == len(tok) == m.count
        assert np.all(np.diff(idx) > 0) and (m.count == 0 or (idx[0] >= 0 and idx[-1] < V * P))          # distinct, sorted, in range
        v, i = idx // P, idx % P
        assert np.array_equal(tok, v * (1 + P + R) + 1 + i)
        for view in np.unique(v):
            n = int((v == view).sum())
            assert max(1, round(ratio[0] * P)) <= n <= max(1, round(ratio[1] * P))                        # exactly a target inside the range
            assert np.all(w[v == view] == np.float32(1.0 / n)) and abs(float(w[v == view].astype(np.float64).sum()) - 1.0) < 1e-6


@pytest.mark.parametrize("grid,n", [(4, 1), (4, 3), (4, 16), (14, 20), (14, 98), (14, 196), (3, 5)])
def test_block_mask_hits_the_count_exactly(grid, n):
    from dinox.ibot import block_mask
    for seed in range(8):
        m = block_mask(np.random.default_rng(seed), grid, n)
        assert m.shape == (grid, grid) and int(m.sum()) == n
    with pytest.raises(ValueError):
        block_mask(np.random.default_rng(0), grid, 0)


def test_same_seed_same_masks_and_prob_zero_masks_nothing():
    from dinox.ibot import MaskGenerator
    a, b, c = (MaskGenerator(s, 14, registers=4) for s in (11, 11, 12))
    da, db, dc = [a.draw(8) for _ in range(3)], [b.draw(8) for _ in range(3)], [c.draw(8) for _ in range(3)]
    assert all(np.array_equal(x.idx, y.idx) and np.array_equal(x.w, y.w) and np.array_equal(x.tok, y.tok) for x, y in zip(da, db))
    assert any(not np.array_equal(x.idx, y.idx) for x, y in zip(da, dc))
    none = MaskGenerator(11, 14, mask_prob=0.0).draw(8)
    assert none.count == 0 and none.to("cpu") is none
    every = MaskGenerator(11, 4, mask_prob=1.0).draw(8)
    assert len(np.unique(every.idx // 16)) == 8
    for bad in (dict(mask_prob=1.5), dict(ratio=(0.0, 0.5)), dict(ratio=(0.6, 0.5)), dict(ratio=(0.1, 1.5))):
        with pytest.raises(ValueError):
            MaskGenerator(0, 4, **bad)


def test_masks_leave_every_other_generator_alone(cli):
    """The view draws of --train-seed come from the process generators (Python, NumPy, torch): drawing masks must not move them."""
    from dinox.ibot import MaskGenerator
    cli._seed_all(5)
    before = (random.getstate(), np.random.get_state(), torch.get_rng_state())
    g = MaskGenerator(5, 14, registers=4)
    for _ in range(4):
        g.draw(16)
    assert random.getstate() == before[0] and torch.equal(torch.get_rng_state(), before[2])
    st = np.random.get_state()
    assert st[0] == before[1][0] and np.array_equal(st[1], before[1][1]) and st[2:] == before[1][2:]


def test_make_mask_rejects_duplicates_and_out_of_range():
    from dinox.ibot import make_mask
    m = make_mask([5, 1, 17], n_views=2, patches=16, registers=2)
    assert list(m.idx) == [1, 5, 17] and list(m.tok) == [2, 6, 19 + 2] and np.allclose(m.w, [0.5, 0.5, 1.0])
    for bad in ([1, 1], [-1], [32]):
        with pytest.raises(ValueError):
            make_mask(bad, 2, 16)


# ------------------------------------------------------------------------------------------ oracle
@pytest.mark.parametrize("regime", ["normal", "underflow", "onehot"])
@pytest.mark.parametrize("M,K", [(1, 8), (5, 1028), (7, 64)])
def test_oracle_equals_literal_autograd(regime, M, K):
    s, t, c = IO.dino_inputs(regime, M, M, K, seed=M + K)
    w = np.random.default_rng(M).uniform(0.0, 1.0, M).astype(np.float32)
    w[M // 2] = 0.0
    o = IO.ibot_ce(s, t, c, w, 0.1, 0.04, scale=1.0 / 6, grad_scale=0.7)
    loss, ds = IO.ibot_ce_torch(s, t, c, w, 0.1, 0.04, scale=1.0 / 6, grad_scale=0.7)
    assert abs(o["loss"] - loss) <= 1e-12 * max(1.0, abs(loss))
    assert np.abs(o["ds"] - ds).max() <= 1e-12 * max(1.0, np.abs(ds).max())
    assert np.all(o["ds"][M // 2] == 0.0)


@pytest.mark.parametrize("regime", ["normal", "underflow", "onehot"])
def test_fp32_evaluation_of_the_oracle_stays_inside_the_bound(regime):
    M, K = 9, 1028
    s, t, c = IO.dino_inputs(regime, M, M, K, seed=3)
    w = np.random.default_rng(1).uniform(0.01, 1.0, M).astype(np.float32)
    o, lo = IO.ibot_ce(s, t, c, w, 0.1, 0.04, 0.25, 0.5), IO.ibot_ce(s, t, c, w, 0.1, 0.04, 0.25, 0.5, dt=np.float32)
    b = IO.bound_ibot(o)
    assert np.all(np.abs(lo["row"] - o["row"]) <= b["row"] + IO.CE_LOSS_RTOL * np.abs(o["row"]))
    assert np.all(np.abs(lo["ds"] - o["ds"]) <= b["ds"] + IO.CE_DS_RTOL * np.abs(o["ds"]).max(1, keepdims=True))
    assert abs(lo["loss"] - o["loss"]) <= b["loss"] + IO.CE_LOSS_RTOL * abs(o["loss"])


@pytest.mark.parametrize("K", [2052, 4096, 4100, 1030, 8196])
@pytest.mark.parametrize("regime", ["normal", "underflow", "onehot"])
def test_fp32_evaluation_stays_inside_the_bound_at_every_row_length_the_gpu_runs(regime, K):
    """The row lengths tests/test_ibot_gpu.py adds for ibot_ce_reg_kernel<4>, <8> with idle groups and the scalar kernel: the bound admits
    correct fp32 arithmetic there before the GPU is asked (M = 5 as there)."""
    M = 5
    s, t, c = IO.dino_inputs(regime, M, M, K, seed=M + K)
    w = np.random.default_rng(M * K).uniform(0.05, 1.0, M).astype(np.float32)
    o, lo = IO.ibot_ce(s, t, c, w, 0.1, 0.04, 1.0 / 6, 0.5), IO.ibot_ce(s, t, c, w, 0.1, 0.04, 1.0 / 6, 0.5, dt=np.float32)
    b = IO.bound_ibot(o)
    assert np.all(np.abs(lo["row"] - o["row"]) <= b["row"] + IO.CE_LOSS_RTOL * np.abs(o["row"]))
    assert np.all(np.abs(lo["ds"] - o["ds"]) <= b["ds"] + IO.CE_DS_RTOL * np.abs(o["ds"]).max(1, keepdims=True))
    assert abs(lo["loss"] - o["loss"]) <= b["loss"] + IO.CE_LOSS_RTOL * abs(o["loss"])


# ------------------------------------------------------------------------------------------ parser, engine, model
def test_parser_flags_and_refusals(cli, monkeypatch):
    monkeypatch.delenv("DINOX_AUTOGRAD_TOP", raising=False)
    d = cli.parse_cli([])                  # (build_ibot_parser: build_parser() keeps the flag surface tests/test_cli_cpu.py pins)
    assert d.ibot_weight == 0.0 and d.ibot_mask_prob == 0.5 and list(d.ibot_mask_ratio) == [0.1, 0.5]
    a = cli.parse_cli(["--ibot-weight", "1.0", "--ibot-mask-prob", "0.3", "--ibot-mask-ratio", "0.2", "0.4"])
    assert a.ibot_weight == 1.0 and a.ibot_mask_prob == 0.3 and list(a.ibot_mask_ratio) == [0.2, 0.4]
    cli.check_loss_type(a)
    cli.check_loss_type(cli.parse_cli(["--hip-graph"]))                                                  # weight 0: nothing to refuse
    for lt in ("simclr", "mae"):
        with pytest.raises(SystemExit, match="--ibot-weight"):
            cli.check_loss_type(cli.parse_cli(["--ibot-weight", "1", "--loss-type", lt, "--mae-decoder", "64x1x2"]))
    with pytest.raises(SystemExit, match="--hip-graph"):
        cli.check_loss_type(cli.parse_cli(["--ibot-weight", "1", "--hip-graph"]))
    monkeypatch.setenv("DINOX_AUTOGRAD_TOP", "1")
    with pytest.raises(SystemExit, match="stock DINO head"):
        cli.check_loss_type(cli.parse_cli(["--ibot-weight", "1"]))
    monkeypatch.delenv("DINOX_AUTOGRAD_TOP")
    for bad in (["--ibot-weight", "-1"], ["--ibot-weight", "1", "--ibot-mask-prob", "1.5"], ["--ibot-weight", "1", "--ibot-mask-ratio", "0.5", "0.2"]):
        with pytest.raises(SystemExit, match="--ibot"):
            cli.check_loss_type(cli.parse_cli(bad))


def test_saved_config_names_the_term_only_when_it_is_on(cli):
    from dataclasses import asdict
    from dinox.engine import StepHyperParams
    cfg = cli.TrainingConfig(model=cli.MODEL_CONFIGS["vit-small"])
    assert cli.config_dict(cfg, StepHyperParams()) == asdict(cfg) and cli.config_dict(cfg, cli.parse_cli([])) == asdict(cfg)
    assert cli.config_dict(cfg, StepHyperParams(ibot_weight=0.5))["ibot_weight"] == 0.5
    assert StepHyperParams().ibot_weight == 0.0


def test_engine_refusals(monkeypatch):
    import zoo.arch as arch
    from dinox.engine import StepHyperParams, TrainEngine
    monkeypatch.delenv("DINOX_AUTOGRAD_TOP", raising=False)
    for hp, kw, word in ((StepHyperParams(ibot_weight=1.0, loss_type="simclr"), {}, "loss_type"),
                         (StepHyperParams(ibot_weight=1.0, loss_type="mae"), {}, "loss_type"),
                         (StepHyperParams(ibot_weight=1.0), dict(use_graph=True), "use_graph"),
                         (StepHyperParams(ibot_weight=-1.0), {}, "ibot_weight")):
        with pytest.raises(ValueError, match=word):
            TrainEngine(None, None, 16, hp, **kw)                          # (before a module or a device is touched)
    vit = dict(img_size=16, patch=8, dim=16, depth=1, heads=2, num_registers=1)

    def pair(mask_token, plain_head=False):
        nets = [arch.DinoStudentTeacher(arch.PatchViT(mask_token=mask_token, **vit), 16) for _ in range(2)]
        if plain_head:
            for n in nets:
                n.head[0] = torch.nn.Linear(16, 16)
        return nets
    with pytest.raises(ValueError, match="stock DINO head"):
        TrainEngine(*pair(True, plain_head=True), 16, StepHyperParams(ibot_weight=1.0))
    with pytest.raises(ValueError, match="mask_token=True"):
        TrainEngine(*pair(False), 16, StepHyperParams(ibot_weight=1.0))
    eng = TrainEngine(*pair(False), 16, StepHyperParams())
    with pytest.raises(ValueError, match="patch_mask"):
        eng.step(torch.zeros(2, 3, 16, 16), patch_mask=(None, None, None))


def test_mask_token_leaves_the_initial_weights_alone():
    import zoo.arch as arch
    kw = dict(img_size=28, patch=14, dim=32, depth=2, heads=2, num_registers=4, scale_aware=True)
    torch.manual_seed(4)
    a = arch.PatchViT(**kw)
    after_a = torch.get_rng_state()
    torch.manual_seed(4)
    b = arch.PatchViT(mask_token=True, **kw)
    assert torch.equal(torch.get_rng_state(), after_a)                     # as many draws: what is built next starts from the same state
    sa, sb = a.state_dict(), b.state_dict()
    assert set(sb) - set(sa) == {"mask_token"} and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert sb["mask_token"].shape == (1, 1, 32) and not sb["mask_token"].any() and "mask_token" not in sa
    with pytest.raises(ValueError, match="mask_token=True"):
        a._forward(torch.zeros(1, 3, 28, 28), None, None, torch.zeros(1, dtype=torch.int32))


def test_load_model_drops_the_training_only_token(tmp_path):
    import zoo.arch as arch
    import zoo.hub as hub
    kw = dict(img_size=28, patch=14, dim=32, depth=1, heads=2, num_registers=4)
    m = arch.DinoStudentTeacher(arch.PatchViT(mask_token=True, **kw), 16)
    with torch.no_grad():
        m.backbone.mask_token.fill_(0.5)
    sd = m.state_dict()
    assert "backbone.mask_token" in sd
    torch.save({"student": sd, "config": {"model": dict(patch=14, dim=32, depth=1, heads=2), "img_size": 28}}, tmp_path / "a.pth")
    torch.save({"student": {k: v for k, v in sd.items() if k != "backbone.mask_token"},
                "config": {"model": dict(patch=14, dim=32, depth=1, heads=2), "img_size": 28}}, tmp_path / "b.pth")
    a, b = hub.load_model(str(tmp_path / "a.pth")), hub.load_model(str(tmp_path / "b.pth"))
    assert list(a.state_dict()) == list(b.state_dict()) and "mask_token" not in a.state_dict()
    assert all(torch.equal(x, y) for x, y in zip(a.state_dict().values(), b.state_dict().values()))


# ------------------------------------------------------------------------------------------ C ABI, host side
def test_entries_reject_bad_arguments_without_a_launch():
    """Every refusal is DINOX_EINVAL from the host-side checks (safe without a GPU: nothing is launched, no pointer is read)."""
    from dinox import _lib
    L, p = _lib.lib, 0x10000
    F32, BF16 = _lib.F32, _lib.BF16
    ok_ce = dict(s=p, t=2 * p, c=3 * p, w=4 * p, ts=0.1, tt=0.04, scale=1.0, gs=1.0, loss=5 * p, ds=6 * p, row=7 * p, M=4, K=8)

    def ce(**kw):
        a = dict(ok_ce, **kw)
        return L.dinox_ibot_ce(a["s"], a["t"], a["c"], a["w"], a["ts"], a["tt"], a["scale"], a["gs"], a["loss"], a["ds"], a["row"], a["M"], a["K"], None)
    for kw in (dict(s=None), dict(t=None), dict(c=None), dict(w=None), dict(loss=None), dict(row=None), dict(M=0), dict(K=0), dict(ts=0.0),
               dict(tt=-1.0), dict(ds=p), dict(ds=2 * p), dict(ds=p + 16)):
        assert ce(**kw) == -1, kw
    assert "alias" in _lib.last_error()
    for dt in (F32, BF16):
        assert L.dinox_ibot_put_mask(None, p, p, 1, 4, 8, dt, None) == -1 and L.dinox_ibot_put_mask(p, None, p, 1, 4, 8, dt, None) == -1
        assert L.dinox_ibot_put_mask(p, p, None, 1, 4, 8, dt, None) == -1
        for M, rows, D in ((0, 4, 8), (1, 0, 8), (1, 4, 0)):
            assert L.dinox_ibot_put_mask(p, p, p, M, rows, D, dt, None) == -1
            assert L.dinox_ibot_put_mask_bwd(p, p, p, p, M, rows, D, dt, None) == -1
            assert L.dinox_gather_rows(p, p, p, M, rows, D, 0, dt, None) == -1
            assert L.dinox_scatter_add_rows(p, p, p, M, rows, D, 0, dt, None) == -1
        for hole in range(4):
            args = [p, p, p, p]
            args[hole] = None
            assert L.dinox_ibot_put_mask_bwd(*args, 1, 4, 8, dt, None) == -1
        for hole in range(3):
            args = [p, p, p]
            args[hole] = None
            assert L.dinox_gather_rows(*args, 1, 4, 8, 0, dt, None) == -1 and L.dinox_scatter_add_rows(*args, 1, 4, 8, 0, dt, None) == -1
        assert L.dinox_gather_rows(p, p, p, 1, 4, 8, -1, dt, None) == -1 and L.dinox_scatter_add_rows(p, p, p, 1, 4, 8, -1, dt, None) == -1
    for dt in (_lib.U16, 7):
        assert L.dinox_ibot_put_mask(p, p, p, 1, 4, 8, dt, None) == -1 and L.dinox_ibot_put_mask_bwd(p, p, p, p, 1, 4, 8, dt, None) == -1
        assert L.dinox_gather_rows(p, p, p, 1, 4, 8, 0, dt, None) == -1 and L.dinox_scatter_add_rows(p, p, p, 1, 4, 8, 0, dt, None) == -1
    assert L.dinox_ibot_center_ema(None, p, 0.9, 8, None) == -1 and L.dinox_ibot_center_ema(p, p, 0.9, 0, None) == -1
    assert L.dinox_version() == 3
