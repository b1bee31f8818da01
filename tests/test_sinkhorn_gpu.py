"""Sinkhorn-Knopp teacher centring on the GPU (csrc/sinkhorn.hip, ops.sk_*, TrainEngine(centering="sinkhorn")).

The primitives and the fused entry are held, element by element, to the bounds of tests/_sinkhorn_oracle.py against its float64
statements (tests/test_sinkhorn_cpu.py shows an fp32 NumPy evaluation inside the same bounds); the centre is also fed to the float64
cross-entropy statement and its row targets compared with the published loop.  Every output buffer starts as NaN.  Each check prints
``ratio <name> <largest error / bound>`` (visible with ``pytest -s``).

The engine tests are bit-for-bit: a step with centering="sinkhorn" is the step of an EMA engine whose centre was set to ops.sk_center of
that batch's teacher logits."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

import _small_kernels_oracle as SO
import _sinkhorn_oracle as SK

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPES = [(1, 8), (2, 5), (6, 64), (7, 257), (33, 4100), (130, 1028)]
REGIMES = ["normal", "onehot", "wide"]


@pytest.fixture(scope="module")
def dx():
    from dinox import ops
    import dinox._lib as L
    assert L.lib.dinox_device_ok() == 1, L.last_error()
    return ops, L


def nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=DEV, dtype=torch.float32)


def off1(t):
    """The same values in storage that starts one float past an aligned address: the launchers must take their scalar kernels."""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=DEV)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0
    return v


def P(t):
    return None if t is None else t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


def host(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def within(name, got, ref, bound):
    got = host(got) if torch.is_tensor(got) else np.asarray(got, np.float64)
    ref, bound = np.broadcast_to(np.asarray(ref, np.float64), got.shape), np.broadcast_to(np.asarray(bound, np.float64), got.shape)
    assert np.isfinite(got).all(), f"{name}: {int((~np.isfinite(got)).sum())} elements not finite (unwritten or overflowed)"
    ratio = float((np.abs(got - ref) / bound).max())
    print(f"ratio {name} {ratio:.4f}")
    assert ratio <= 1.0, f"{name}: error at {ratio:.3f} of the bound (worst element {int(np.argmax(np.abs(got - ref) / bound))})"


_INPUTS = {}


def inputs(regime, R, K):
    """(t fp32, tau, its device copy): drawn once per (regime, shape), shared by every test that needs it and never written to."""
    key = (regime, R, K)
    if key not in _INPUTS:
        t, tt = SK.sk_inputs(regime, R, K, seed=R + K)
        td = dev(t)
        t.setflags(write=False)
        _INPUTS[key] = (t, tt, td)
    return _INPUTS[key]


_CENTERS = {}


def center_ref(regime, R, K, iters):
    key = (regime, R, K, iters)
    if key not in _CENTERS:
        t, tt, _ = inputs(regime, R, K)
        _CENTERS[key] = SK.bound_center(t, tt, iters)
    return _CENTERS[key]


def ws_for(L, R, K):
    return nan(int(L.lib.dinox_sk_ws_floats(R, K)))


def col_lse(L, t, a, inv, scale=1.0):
    R, K = t.shape
    out = nan(K)
    L.check(L.lib.dinox_sk_col_lse(P(t), P(a), inv, scale, P(out), P(ws_for(L, R, K)), R, K, stream()), "dinox_sk_col_lse")
    return out


def row_lse(L, t, b, inv, scale=1.0):
    R, K = t.shape
    out = nan(R)
    L.check(L.lib.dinox_sk_row_lse(P(t), P(b), inv, scale, P(out), R, K, stream()), "dinox_sk_row_lse")
    return out


def center(L, t, tt, iters):
    R, K = t.shape
    out = nan(K)
    L.check(L.lib.dinox_sk_center(P(t), tt, iters, P(out), P(ws_for(L, R, K)), R, K, stream()), "dinox_sk_center")
    return out


# ========================================================================================== primitives
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("R,K", SHAPES)
def test_primitives_against_fp64(dx, R, K, regime):
    """K % 4 == 0 and aligned: the float4 kernels ((1, 8): fewer columns than one workgroup owns; 4100 and 1028: more than one column
    workgroup); K = 5, 257 and every view one float off alignment: the scalar kernels.  R = 1 .. 7: rows missing in the slices of the
    one chunk; 33: a second chunk with one row; 130: five chunks, the last with two rows.  a / b NULL and drawn around minus the row
    (column) maximum, which is where the recurrence puts them."""
    _, L = dx
    t, tt, td = inputs(regime, R, K)
    inv = SK.inv_temp(tt)
    r = np.random.default_rng(R * K)
    z = t.astype(np.float64) * inv
    a = (-z.max(1) + 3 * r.standard_normal(R)).astype(np.float32)
    b = (-z.max(0) + 3 * r.standard_normal(K)).astype(np.float32)
    for tag, tv in (("", td), (".off1", off1(td))):
        for av in (None, a):
            ref, parts = SK.col_pass(t, av, inv)
            within(f"sk_col_lse{tag}.{'a' if av is not None else 'null'}", col_lse(L, tv, None if av is None else dev(av), inv), ref, SK.bound_pass(parts))
        for bv in (None, b):
            ref, parts = SK.row_pass(t, bv, inv)
            within(f"sk_row_lse{tag}.{'b' if bv is not None else 'null'}", row_lse(L, tv, None if bv is None else dev(bv), inv), ref, SK.bound_pass(parts))
    # b one float off alignment beside an aligned t: the row pass must drop to its scalar kernel too
    ref, parts = SK.row_pass(t, b, inv)
    within("sk_row_lse.b_off1", row_lse(L, td, off1(dev(b)), inv), ref, SK.bound_pass(parts))
    # the output scale is one exact or once-rounded product
    ref, parts = SK.col_pass(t, a, inv)
    within("sk_col_lse.scaled", col_lse(L, td, dev(a), inv, -1.0), -ref, SK.bound_pass(parts))


# ========================================================================================== the fused entry
@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("R,K", SHAPES)
def test_center_against_the_oracle_and_the_published_loop(dx, R, K, regime, iters):
    """The centre inside its carried bound; and, fed to the float64 cross-entropy statement, row targets that are the published loop's
    Q within what that bound allows (the loop runs in long double: exp(t / tau) leaves float64 in the onehot regime)."""
    ops, L = dx
    t, tt, td = inputs(regime, R, K)
    c_ref, bound = center_ref(regime, R, K, iters)
    got = center(L, td, tt, iters)
    within(f"sk_center.{regime}.{iters}", got, c_ref, bound)
    assert torch.equal(ops.sk_center(td, tt, iters), got)                   # the wrapper is that call
    wide = np.finfo(np.longdouble).maxexp > np.finfo(np.float64).maxexp
    if not wide and float(np.abs(t).max()) / tt > 300:
        return                                                              # long double is float64 on this host: the linear-domain loop has no finite statement here
    q = SK.sk_literal(t, tt, iters, dt=np.longdouble if wide else np.float64).astype(np.float64)
    assert np.isfinite(q).all() and np.abs(q.sum(1) - 1).max() < 1e-9
    tp = SO.dino_ce(t, t, host(got), 0.1, tt)["tp"]
    within(f"sk_targets.{regime}.{iters}", tp, q, SK.bound_targets(q, bound, tt))


def test_center_is_deterministic(dx):
    _, L = dx
    for R, K in ((130, 1028), (33, 4100), (7, 257)):
        _, tt, td = inputs("normal", R, K)
        assert torch.equal(center(L, td, tt, 3), center(L, td, tt, 3))
        assert torch.equal(col_lse(L, td, None, 25.0), col_lse(L, td, None, 25.0))


@pytest.mark.parametrize("R,K", [(130, 1028), (7, 257)])
def test_shard_identity(dx, R, K):
    """The data-parallel building block on one GPU: the rows in two shards, every column pass run per shard, the two K-vectors stacked
    to [2][K] and met by sk_col_lse (inv_temp 1, a NULL); the row passes per shard.  Log-sum-exp of the shards' log-sum-exps is the
    log-sum-exp of all rows, so the centre equals the fused entry's within twice the single-rank bound."""
    _, L = dx
    t, tt, td = inputs("normal", R, K)
    inv = SK.inv_temp(tt)
    shards = [td[:R // 2].contiguous(), td[R // 2:].contiguous()]
    a = [None, None]
    for n in (1, 2, 3):
        stack = torch.stack([col_lse(L, s, ai, inv) for s, ai in zip(shards, a)])
        if n == 3:
            c = col_lse(L, stack, None, 1.0, tt)
            break
        b = col_lse(L, stack, None, 1.0, -1.0)
        a = [row_lse(L, s, b, inv, -1.0) for s in shards]
    c_ref, bound = center_ref("normal", R, K, 3)
    fused = center(L, td, tt, 3)
    within("sk_shards.vs_fused", c, host(fused), 2 * bound)
    within("sk_shards.vs_fp64", c, c_ref, 2 * bound)


# ========================================================================================== engine
KW = dict(img_size=56, patch=14, dim=64, depth=2, heads=2, num_registers=4, scale_aware=True)
OUT, B = 256, 4


def _state(arch):
    torch.manual_seed(11)
    ref = arch.DinoStudentTeacher(arch.PatchViT(**KW), OUT)
    torch.nn.init.xavier_uniform_(ref.backbone.scale_embed.mlp[2].weight)
    return {k: v.clone() for k, v in ref.state_dict().items()}


def _engine(arch, sd, centering, **kw):
    from dinox.engine import StepHyperParams, TrainEngine
    student, teacher = arch.DinoStudentTeacher(arch.PatchViT(**KW), OUT), arch.DinoStudentTeacher(arch.PatchViT(**KW), OUT)
    student.load_state_dict(sd)
    teacher.load_state_dict(sd)
    hp = StepHyperParams(lr=1e-3, warmup_steps=2, max_steps=8, ema=0.9, koleo_weight=0.1, centering=centering)
    eng = TrainEngine(student.to(DEV), teacher.to(DEV), OUT, hp, **kw)
    student.train()
    return eng


def _batch(seed, crops=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2 * B, 3, 56, 56, generator=g).to(DEV)
    sp = (torch.rand(B, 3, generator=g) + 0.5)
    loc = torch.randn(crops * B, 3, 28, 28, generator=g).to(DEV) if crops else None
    lsp = sp.repeat(crops, 1).to(DEV) if crops else None
    return x, sp.repeat(2, 1).to(DEV), loc, lsp


def _teacher_logits(ops, eng, x, sp):
    """The teacher's logits of a batch through the calls the engine's step makes."""
    with torch.no_grad(), ops.compute_dtype(eng.compute_dtype), ops.unfold_share():
        t_feats = eng.teacher.backbone(x, spacing=sp)
        if eng.manual_top:
            return eng._head(eng.teacher.head, ops.take_rows(t_feats, 0, eng.compute_dtype), train=False)[0]
        return eng.teacher.head(t_feats[:, 0])


@pytest.mark.parametrize("top", ["manual", "autograd"])
@pytest.mark.parametrize("crops", [0, 2], ids=["global", "crops2"])
def test_engine_step_is_the_ema_step_with_the_sinkhorn_centre(dx, monkeypatch, crops, top):
    """Tests A (two global views) and B (plus 2 local crops of side 28; the teacher's 2 B rows are one Sinkhorn-Knopp problem)."""
    ops, _ = dx
    import zoo.arch as arch
    if top == "autograd":
        monkeypatch.setenv("DINOX_AUTOGRAD_TOP", "1")
    sd = _state(arch)
    x, sp, loc, lsp = _batch(3, crops)
    sk, ema = _engine(arch, sd, "sinkhorn"), _engine(arch, sd, "ema")
    assert sk.manual_top == (top == "manual")
    t_out = _teacher_logits(ops, ema, x, sp)
    assert tuple(t_out.shape) == (2 * B, OUT)
    c = ops.sk_center(t_out, ema.hp.teacher_temp, 3)
    assert bool(torch.isfinite(c).all()) and float(c.abs().max()) > 0
    ema.center.copy_(c.view(1, -1))
    # the sinkhorn engine's own EMA centre stays at its initial zeros: were its targets to read it, it would be the zero-centre engine below
    assert float(sk.center.abs().max()) == 0.0
    sk.step(x, sp, loc, lsp)
    ema.step(x, sp, loc, lsp)
    zero = _engine(arch, sd, "ema")
    zero.step(x, sp, loc, lsp)
    a, b, z = sk.scalars(), ema.scalars(), zero.scalars()
    assert list(a) == list(b)                                               # the same keys in both modes
    assert a["loss"] == b["loss"] and a["dino"] == b["dino"] and a["grad_norm"] == b["grad_norm"] and np.isfinite(a["loss"])
    assert torch.equal(sk.flat_p, ema.flat_p) and torch.equal(sk.flat_t, ema.flat_t)
    assert a["dino"] != z["dino"] and not torch.equal(sk.flat_p, zero.flat_p)       # the centre matters, and it is not the engine's own
    # the EMA centre is maintained as ever: from zeros it is the zero-centre EMA engine's, from c the twin's
    assert torch.equal(sk.center, zero.center) and float(sk.center.abs().max()) > 0
    sk_c = _engine(arch, sd, "sinkhorn")
    sk_c.center.copy_(c.view(1, -1))
    sk_c.step(x, sp, loc, lsp)
    assert torch.equal(sk_c.center, ema.center) and not torch.equal(sk_c.center.view(-1), c)
    assert sk_c.scalars()["dino"] == a["dino"] and torch.equal(sk_c.flat_p, sk.flat_p)      # ... and is not read by the targets


def test_engine_graph_replay_equals_eager_bitwise(dx):
    """Test C: Sinkhorn-Knopp is part of the captured step (no allocation outside the pool, no synchronisation, no host-read scalar)."""
    import zoo.arch as arch
    sd = _state(arch)
    batches = [_batch(20 + i)[:2] for i in range(4)]
    runs = []
    for graph in (False, True):
        eng = _engine(arch, sd, "sinkhorn", use_graph=graph)
        out = []
        for x, sp in batches:
            eng.step(x, sp)
            sc = eng.scalars()
            out.append((sc["loss"], sc["dino"], sc["grad_norm"]))
        assert (eng._graph is not None) == graph and eng.opt_steps == 4
        runs.append((out, eng.flat_p.clone(), eng.flat_t.clone(), eng.center.clone()))
    (oe, pe, te, ce), (og, pg, tg, cg) = runs
    assert oe == og and len({l for l, _, _ in og}) == 4 and all(np.isfinite(v) for row in og for v in row)
    assert torch.equal(pe, pg) and torch.equal(te, tg) and torch.equal(ce, cg)


def test_gradient_accumulation_runs_sinkhorn_per_micro_batch(dx):
    """accumulation_steps = 2: each micro-batch is centred by its own Sinkhorn-Knopp problem -- the two dino terms are those of two
    one-step engines' first steps, given the same weights (no optimiser step lies between them)."""
    import zoo.arch as arch
    sd = _state(arch)
    (x0, s0, _, _), (x1, s1, _, _) = _batch(40), _batch(41)
    acc = _engine(arch, sd, "sinkhorn", accumulation_steps=2)
    acc.step(x0, s0)
    d0 = acc.scalars()["dino"]
    acc.step(x1, s1)
    d1 = acc.scalars()["dino"]
    one = _engine(arch, sd, "sinkhorn")
    one.step(x1, s1)
    first = _engine(arch, sd, "sinkhorn")
    first.step(x0, s0)
    assert d0 == first.scalars()["dino"] and d1 == one.scalars()["dino"] and d0 != d1 and acc.opt_steps == 1


# ========================================================================================== RCCL surface at world 1
def test_rccl_call_surface_world1(tmp_path):
    """ops.sk_center(t, group=...) with its all-gathers through the real RCCL backend in a world of one rank equals ops.sk_center(t)
    bit for bit (the log-sum-exp over one gathered row is that row), and an engine step with centering="sinkhorn" runs through it."""
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    worker = os.path.join(ROOT, "tests", "_sk_dp_worker.py")
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
               DINOX_DP_FORCE_COLLECTIVES="1")
    env.pop("DINOX_DIST_BACKEND", None)
    out = str(tmp_path / "sk.pt")
    r = subprocess.run([sys.executable, worker, out], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-2000:]
    got = torch.load(out)
    assert got["backend"] == "nccl" and got["exchanging"]
    for key in ("c1", "c3", "c3_odd"):
        plain, grouped = got[key]
        assert bool(torch.isfinite(plain).all()) and torch.equal(plain, grouped), key
    assert all(np.isfinite(v) for v in got["scalars"].values()) and got["scalars"]["dino"] > 0
    assert got["scalars"] == got["scalars_plain"]                           # the step itself: bit for bit the run without a process group
