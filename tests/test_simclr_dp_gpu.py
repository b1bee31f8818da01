"""Data-parallel SimCLR on the device: the rectangular NT-Xent kernels (local rows x global columns) with the ranks emulated on one GPU,
against the float64 oracle of the global batch and against the square single-rank path; world = 1 through the rectangular path; the
error paths; two ranks over gloo against one process at the whole batch; the RCCL call surface in a world of one; the engine with
simclr_negatives="global" on one rank.

The bar is the project's NT-Xent bar (tests/test_simclr_gpu.py): loss within 1e-3 relative, every gradient row within 1e-3 of that row's
max-abs, rows whose oracle gradient is zero exactly zero, everything finite.  The element-wise judge of the kernels themselves
(a-priori fp32 bounds per kernel, hostile S) is tests/test_ntxent_bounds_gpu.py."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden, sub, t

import _ntxent_dp_oracle as DP
import _ntxent_oracle as NX

pytestmark = pytest.mark.gpu

DEV = "cuda"
TAU = 0.1
# (world, Bl, D): scalar paths with Mg under one tile; Ml = 34 crosses the 32-tile and Mg = 102 is ragged; Ml = 260 exceeds the
# 256-thread sweep (seeded rows: the b130 fixture is 130 x 257, i.e. not 2 x 130 pairs of 256 columns); that fixture split in two
# (Mg = 260 columns per row: more than one 256-thread stride, D % 4 != 0); the adversarial fixture split in two (a duplicated pair and
# the row below eps on rank 0, the all-zero row on rank 1, the parallel rows z1[3], z1[4] one on each rank).
CASES = {"w2_b3_d5": (2, 3, 5), "w3_b17_d64": (3, 17, 64), "w2_b130_d256": (2, 130, 256), "b130_split": (2, 65, 257), "adv_split": (2, 4, 16)}


@pytest.fixture(scope="module")
def dx():
    from dinox import ops
    import dinox._lib as L
    assert L.lib.dinox_device_ok() == 1, L.last_error()
    return ops, L


@pytest.fixture(scope="module")
def gold():
    return load_golden("simclr_loss.npz")


@pytest.fixture(scope="module")
def inputs(gold):
    """tag -> (z1, z2) float32 [B, D] of the global batch, built once and never written."""
    out = {}
    for tag, (world, Bl, D) in CASES.items():
        if tag.endswith("_split"):
            z1, z2 = gold[f"{tag[:-6]}_z1"], gold[f"{tag[:-6]}_z2"]
            assert z1.shape == (world * Bl, D)
        else:
            rng = np.random.default_rng(world * 1000 + Bl)
            z1, z2 = (2.0 * rng.standard_normal((2, world * Bl, D))).astype(np.float32)
        out[tag] = (z1, z2)
    return out


@pytest.fixture(scope="module")
def oracle(inputs):
    """float64 loss and gradient of the global batch [z1; z2] per case, computed once."""
    return {tag: NX.ntxent(np.concatenate([z1, z2], 0), TAU) for tag, (z1, z2) in inputs.items()}


def row_err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = np.abs(want).max(1)
    err = np.abs(got - want).max(1)
    zero = scale == 0
    return float((err[~zero] / scale[~zero]).max()), float(err[zero].max()) if zero.any() else 0.0


def emulate_ranks(ops, L, shards, gscale=1.0):
    """What ``world`` ranks compute, in a loop on one device: normalise per shard, concatenate (the all-gather), then rows_rect and
    coeff_rect per shard with its row0.  Returns (loss, [dz per rank], [lse per rank])."""
    st = torch.cuda.current_stream().cuda_stream
    f = lambda *sh: torch.empty(sh, dtype=torch.float32, device=DEV)
    world, (Ml, D) = len(shards), shards[0].shape
    Mg, Bl, inv_tau = world * Ml, Ml // 2, 1.0 / TAU
    unit = []
    for z in shards:
        z = torch.from_numpy(np.ascontiguousarray(z)).to(DEV)
        zh, norm, sq = f(Ml, D), f(Ml), f(Ml)
        L.check(L.lib.dinox_koleo_normalize(z.data_ptr(), zh.data_ptr(), norm.data_ptr(), sq.data_ptr(), Ml, D, 1e-12, st), "normalize")
        unit.append((zh, norm))
    zh_all = torch.cat([zh for zh, _ in unit], 0)
    S, lses, parts = [], [], f(world)
    for r, (zh, _) in enumerate(unit):
        S.append(ops.gemm_nt_f32_splitk(zh, zh_all))
        assert tuple(S[r].shape) == (Ml, Mg)
        lse, row_loss = f(Ml), f(Ml)
        L.check(L.lib.dinox_ntxent_rows_rect(S[r].data_ptr(), Mg, Ml, Mg, r * Ml, Bl, inv_tau, lse.data_ptr(), row_loss.data_ptr(),
                                             parts.data_ptr() + 4 * r, st), "rows_rect")
        lses.append(lse)
    lse_all = torch.cat(lses, 0)
    total = parts[0:1].clone()
    for r in range(1, world):
        total += parts[r:r + 1]
    loss = float(total / float(Mg))
    dz = []
    for r, (zh, norm) in enumerate(unit):
        W = f(Ml, Mg)
        L.check(L.lib.dinox_ntxent_coeff_rect(S[r].data_ptr(), Mg, lses[r].data_ptr(), lse_all.data_ptr(), Ml, Mg, r * Ml, Bl, inv_tau, gscale,
                                              W.data_ptr(), Mg, st), "coeff_rect")
        dzh = ops.gemm(W, zh_all, transB=True, out_dtype=torch.float32)
        d = f(Ml, D)
        L.check(L.lib.dinox_normalize_bwd(dzh.data_ptr(), zh.data_ptr(), norm.data_ptr(), d.data_ptr(), Ml, D, 1e-12, st), "normalize_bwd")
        dz.append(d.cpu().numpy())
    return loss, dz, [l.cpu().numpy() for l in lses]


@pytest.mark.parametrize("tag", list(CASES))
def test_shards_on_one_device_match_the_global_batch(dx, inputs, oracle, tag):
    """Shard identity: the ranks' losses add up to the NT-Xent of the global batch and their gradients, laid back into the global row
    order and divided by ``world`` (the gradient convention), are its gradient -- against the float64 oracle and against the square
    single-rank kernels on the permuted global batch [z1 of all ranks; z2 of all ranks]."""
    ops, L = dx
    world = CASES[tag][0]
    z1, z2 = inputs[tag]
    loss, dz, lse = emulate_ranks(ops, L, DP.split(z1, z2, world))
    got = DP.unsplit(dz) / world
    assert np.isfinite(loss) and np.isfinite(got).all()
    sq_loss, saved = ops.ntxent_fwd(torch.from_numpy(np.concatenate([z1, z2], 0)).to(DEV), TAU)
    sq_dz = ops.ntxent_bwd(saved, 1.0).cpu().numpy()
    for name, want_loss, want_dz in (("oracle", *oracle[tag]), ("square path", float(sq_loss), sq_dz)):
        e_row, e_zero = row_err(got, want_dz)
        print(f"{tag} vs {name}: loss rel err {abs(loss - want_loss) / abs(want_loss):.2e}, worst gradient row {e_row:.2e}")
        assert abs(loss - want_loss) <= 1e-3 * abs(want_loss)
        assert e_row <= 1e-3 and e_zero == 0.0
    # the lse every rank gathers is the global batch's, row for row (what the transposed term of the other ranks reads)
    sq_lse = saved[3].cpu().numpy()
    assert np.abs(DP.unsplit(lse) - sq_lse).max() <= 1e-3 * max(1.0, float(np.abs(sq_lse).max()))
    # an upstream factor scales the gradient and nothing else
    _, dz4, _ = emulate_ranks(ops, L, DP.split(z1, z2, world), gscale=0.25)
    assert row_err(DP.unsplit(dz4) / world, 0.25 * oracle[tag][1])[0] <= 1e-3


@pytest.mark.parametrize("tag", ["b3", "b33", "b130", "adv"])
def test_world_one_through_the_rectangular_path(dx, gold, tag):
    """force_rect=True: the rectangular kernels with world = 1, row0 = 0 meet the square path at the bar (the same S, hence the same lse
    bit for bit; W takes S_ij for S_ji), and a second call reproduces the first bit for bit."""
    ops, _ = dx
    z = torch.from_numpy(np.concatenate([gold[f"{tag}_z1"], gold[f"{tag}_z2"]], 0)).to(DEV)
    sq_loss, sq_saved = ops.ntxent_fwd(z, TAU)
    sq_dz = ops.ntxent_bwd(sq_saved, 1.0)
    runs = []
    for _ in range(2):
        loss, saved = ops.ntxent_fwd(z.clone(), TAU, force_rect=True)
        runs.append((loss.clone(), ops.ntxent_bwd(saved, 1.0), saved[3].clone()))
    assert len(saved) == 6 and len(sq_saved) == 5
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert torch.equal(runs[0][2], sq_saved[3])
    loss, dz = float(runs[0][0]), runs[0][1].cpu().numpy()
    assert np.isfinite(loss) and np.isfinite(dz).all()
    e_row, e_zero = row_err(dz, sq_dz.cpu().numpy())
    print(f"{tag}: rect vs square loss rel err {abs(loss - float(sq_loss)) / abs(float(sq_loss)):.2e}, worst gradient row {e_row:.2e}")
    assert abs(loss - float(sq_loss)) <= 1e-3 * abs(float(sq_loss))
    assert e_row <= 1e-3 and e_zero == 0.0
    o_loss, o_dz = NX.ntxent(z.cpu().numpy(), TAU)
    assert abs(loss - o_loss) <= 1e-3 * abs(o_loss) and row_err(dz, o_dz)[0] <= 1e-3


def test_autograd_path_equals_manual_path_bitwise(dx, gold):
    ops, _ = dx
    z1 = torch.from_numpy(gold["b33_z1"]).to(DEV).requires_grad_(True)
    z2 = torch.from_numpy(gold["b33_z2"]).to(DEV).requires_grad_(True)
    loss = ops.simclr_loss(z1, z2, TAU, force_rect=True)
    g1, g2 = torch.autograd.grad(loss, [z1, z2])
    m_loss, saved = ops.ntxent_fwd(torch.cat([z1.detach(), z2.detach()], 0), TAU, force_rect=True)
    dz = ops.ntxent_bwd(saved, 1.0)
    assert loss.dim() == 0 and torch.equal(loss.detach().reshape(1), m_loss)
    assert torch.equal(g1, dz[:33]) and torch.equal(g2, dz[33:])


def test_error_paths_launch_nothing(dx):
    """Odd Ml, Mg not a multiple of Ml, a misaligned row0 and inv_tau <= 0 on real device buffers: the error code, and the outputs as
    they were."""
    _, L = dx
    S = torch.randn(8, 16, device=DEV)
    out = torch.full((24,), -7.0, device=DEV)
    W = torch.full((8, 16), -7.0, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    lse, row_loss, part = out.data_ptr(), out.data_ptr() + 32, out.data_ptr() + 64
    good = dict(Ml=8, Mg=16, row0=8, Bl=4, inv_tau=10.0)
    for bad, word in ((dict(Ml=7, Bl=3), "Ml=7"), (dict(Mg=12), "Mg=12"), (dict(row0=4), "row0=4"), (dict(row0=16), "row0=16"),
                      (dict(inv_tau=0.0), "inv_tau"), (dict(inv_tau=-10.0), "inv_tau"), (dict(Bl=3), "Bl=3")):
        a = dict(good, **bad)
        assert L.lib.dinox_ntxent_rows_rect(S.data_ptr(), 16, a["Ml"], a["Mg"], a["row0"], a["Bl"], a["inv_tau"], lse, row_loss, part, st) == -1
        assert word in L.last_error(), (bad, L.last_error())
        assert L.lib.dinox_ntxent_coeff_rect(S.data_ptr(), 16, lse, lse, a["Ml"], a["Mg"], a["row0"], a["Bl"], a["inv_tau"], 1.0,
                                             W.data_ptr(), 16, st) == -1
        assert word in L.last_error(), (bad, L.last_error())
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((W == -7.0).all())
    # and the good arguments do launch
    assert L.lib.dinox_ntxent_rows_rect(S.data_ptr(), 16, 8, 16, 8, 4, 10.0, lse, row_loss, part, st) == 0
    torch.cuda.synchronize()
    assert bool((out[:17] != -7.0).all()) and bool((out[17:] == -7.0).all())


# ------------------------------------------------------------------------------------------ processes
def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    return port


WORKER = os.path.join(ROOT, "tests", "_simclr_dp_worker.py")


def test_two_ranks_match_single_process(dx, tmp_path):
    """Two ranks (gloo, both on this GPU -- RCCL needs one GPU per rank) take two steps with simclr_negatives="global" on their shard of
    a global batch of 8, from different seeds; one process takes them at the whole batch on the square kernels.  Same loss (already
    global: the same bits on both ranks), same gradient norm, same weights -- the bands of
    test_engine_data_parallel_two_ranks_match_single_process."""
    outs = [str(tmp_path / f"r{r}.pt") for r in range(2)]
    env = dict(os.environ, DINOX_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), WORLD_SIZE="2")
    env.pop("DINOX_DP_FORCE_COLLECTIVES", None)
    procs = [subprocess.Popen([sys.executable, WORKER, "steps", outs[r]], env=dict(env, RANK=str(r), LOCAL_RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(2)]
    logs = [p.communicate(timeout=240)[0].decode(errors="replace")[-1500:] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)
    single = subprocess.run([sys.executable, WORKER, "steps", str(tmp_path / "single.pt")], env=dict(env, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"),
                            stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    assert single.returncode == 0, single.stdout.decode(errors="replace")[-1500:]
    a, b, ref = torch.load(outs[0]), torch.load(outs[1]), torch.load(tmp_path / "single.pt")
    assert torch.equal(a["flat_p"], b["flat_p"])                                      # the ranks stay in lock-step
    assert a["loss"] == b["loss"] and a["simclr"] == a["loss"] and np.isfinite(a["loss"])
    print(f"loss {a['loss']:.6f} vs single {ref['loss']:.6f}; grad-norm {a['grad_norm']:.5f} / {b['grad_norm']:.5f} vs {ref['grad_norm']:.5f}")
    assert a["loss"] == pytest.approx(ref["loss"], rel=2e-4)
    assert a["grad_norm"] == pytest.approx(ref["grad_norm"], rel=2e-3) and b["grad_norm"] == a["grad_norm"]
    d = (a["flat_p"] - ref["flat_p"]).abs()
    assert float((d <= 1e-5 + 1e-4 * ref["flat_p"].abs()).double().mean()) > 0.995     # Adam sign-noise on ~zero grads aside
    assert float(d.max()) <= 2.5e-3


def test_rccl_call_surface_world1(dx, tmp_path):
    """ops.ntxent_fwd / ntxent_bwd with their three all-gathers through the real RCCL backend in a world of one rank, and one engine step
    with simclr_negatives="global", against the same calls without a process group (the square kernels), at the bar."""
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()),
               DINOX_DP_FORCE_COLLECTIVES="1")
    env.pop("DINOX_DIST_BACKEND", None)
    out = str(tmp_path / "surface.pt")
    r = subprocess.run([sys.executable, WORKER, "surface", out], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-2000:]
    got = torch.load(out)
    assert got["backend"] == "nccl" and got["exchanging"]
    (p_loss, p_dz, p_n), (u_loss, u_dz, u_n), (g_loss, g_dz, g_n) = got["plain"], got["ungrouped"], got["grouped"]
    assert (p_n, u_n, g_n) == (5, 5, 6)                                              # the group, and only the group, selects the rectangular path
    assert torch.equal(p_loss, u_loss) and torch.equal(p_dz, u_dz)
    assert bool(torch.isfinite(g_loss).all()) and bool(torch.isfinite(g_dz).all())
    e_row, e_zero = row_err(g_dz.numpy(), p_dz.numpy())
    print(f"grouped vs plain: loss {float(g_loss):.6f} vs {float(p_loss):.6f}, worst gradient row {e_row:.2e}")
    assert abs(float(g_loss) - float(p_loss)) <= 1e-3 * abs(float(p_loss)) and e_row <= 1e-3 and e_zero == 0.0
    sc, sp = got["scalars"], got["scalars_plain"]
    assert set(sc) == set(sp) and all(np.isfinite(v) for v in sc.values()) and sc["simclr"] == sc["loss"] > 0
    for k in sc:
        assert sc[k] == pytest.approx(sp[k], rel=1e-3), (k, sc[k], sp[k])


# ------------------------------------------------------------------------------------------ the engine on one rank
def _cfg(arr):
    img, patch, dim, depth, heads, regs, sa, out = [int(v) for v in arr]
    return dict(img_size=img, patch=patch, dim=dim, depth=depth, heads=heads, num_registers=regs, scale_aware=bool(sa)), out


@pytest.mark.parametrize("top", ["manual", "autograd"])
def test_engine_global_negatives_on_one_rank(dx, monkeypatch, top):
    """simclr_negatives="global" in a world of one rank has nothing to gather: three steps from tests/golden/simclr_step_tiny.npz meet the
    reference's gradients of every step at the bound of test_engine_three_steps_match_the_reference (1e-3 of each tensor's max-abs
    + 1e-7), and leave the weights the "local" engine leaves, bit for bit.  Both tops."""
    import zoo.arch as arch
    from dinox.engine import StepHyperParams, TrainEngine
    if top == "autograd":
        monkeypatch.setenv("DINOX_AUTOGRAD_TOP", "1")
    else:
        monkeypatch.delenv("DINOX_AUTOGRAD_TOP", raising=False)
    g = load_golden("simclr_step_tiny.npz")
    cfg, out_dim = _cfg(g["cfg"])
    lr, min_lr, warm, max_steps, wd, temp = [float(v) for v in g["hp"]]
    init = {k: v.float() for k, v in sub(g, "init").items()}
    arenas = {}
    for negatives in ("global", "local"):
        hp = StepHyperParams(lr=lr, min_lr=min_lr, warmup_steps=int(warm), max_steps=int(max_steps), weight_decay=wd, loss_type="simclr",
                             simclr_temp=temp, simclr_negatives=negatives)
        student = arch.DinoStudentTeacher(arch.PatchViT(**cfg), out_dim)
        teacher = arch.DinoStudentTeacher(arch.PatchViT(**cfg), out_dim)
        student.load_state_dict(init)
        teacher.load_state_dict(init)
        eng = TrainEngine(student.to(DEV), teacher.to(DEV), out_dim, hp)
        assert eng.manual_top == (top == "manual")
        for step in range(3):
            eng.step(t(g[f"batch{step}"]).float().to(DEV), t(g[f"spacing{step}"]).to(DEV))
            r = eng.scalars()
            assert r["loss"] == pytest.approx(float(g["losses"][step]), rel=1e-3) and r["simclr"] == r["loss"]
            worst = (0.0, "")
            for n, p in student.named_parameters():
                want = t(g[f"grad{step}/{n}"]).double()
                err = float((p.grad.cpu().double() - want).abs().max())
                bound = 1e-3 * float(want.abs().max()) + 1e-7
                worst = max(worst, (err / bound, n))
                assert err <= bound, (negatives, step, n, err, bound)
            print(f"{negatives}, step {step}: worst tensor {worst[1]} at {worst[0]:.3f} of its bound")
        arenas[negatives] = eng.flat_p.clone()
    assert torch.equal(arenas["global"], arenas["local"])
