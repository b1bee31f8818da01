"""GPU tests of the fused similarity-rank kernel (csrc/retrieval.hip) and the view-retrieval evaluation built on it
(dinox/retrieval.py, scripts/phase5_view_retrieval_eval.py).  Run with ``-m gpu`` on an MI355X.

1. exact case: integer-valued fp32 rows in {-3..3} make every partial sum an integer far below 2^24, so every score is exact in
   fp32 and the four outputs must EQUAL integer arithmetic on the host -- no tolerance; ties are frequent, so the tie rule works;
2. float case: clustered unit rows against a float64 product, with the per-row rank interval that the fp32 chain error allows;
3. self-consistency: best_idx fed back as target, bitwise-duplicated keys, run-to-run identity;
4. end to end: embeddings against the CPU oracle, metrics against a float64 ranking of the engine's own embeddings, the script
   on a reference-written checkpoint.
"""
import json
import os
import random
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from dinox import ops
    import dinox._lib as L
    assert L.lib.dinox_device_ok() == 1, L.last_error()
    return ops


def run_rank(ops, q, k, target=None):
    tq, tk = torch.from_numpy(q).to(DEV), torch.from_numpy(k).to(DEV)
    tt = None if target is None else torch.from_numpy(target.astype(np.int32)).to(DEV)
    out = ops.retrieval_rank(tq, tk, tt)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]           # rank, best_idx, best_val, pos_val


def stable_ranks(S, target):
    """#{j : S[i,j] > S[i,t_i]} + #{j < t_i : S[i,j] == S[i,t_i]}: the place of t_i in a stable descending sort of row i."""
    pos = S[np.arange(S.shape[0]), target][:, None]
    before = np.arange(S.shape[1])[None, :] < target[:, None]
    return ((S > pos) | ((S == pos) & before)).sum(1)


# ------------------------------------------------------------------------------------------ 1. exact
EXACT_SHAPES = [(4096, 4096, 384), (777, 1029, 384), (129, 4099, 1024), (1000, 1000, 88), (1, 1, 1), (300, 65, 7)]


def integer_rows(Nq, Nk, D):
    g = np.random.default_rng(Nq * 7 + Nk * 3 + D)
    q = g.integers(-3, 4, (Nq, D)).astype(np.float32)
    k = g.integers(-3, 4, (Nk, D)).astype(np.float32)
    # integer arithmetic: |s| <= 9 D < 2^14 and every partial sum is an integer, so the float64 BLAS product is the exact int64 result
    S = (q.astype(np.float64) @ k.astype(np.float64).T).astype(np.int64)
    return g, q, k, S


@pytest.mark.parametrize("Nq,Nk,D", EXACT_SHAPES)
def test_exact_integer_scores(ops, Nq, Nk, D):
    g, q, k, S = integer_rows(Nq, Nk, D)
    if Nq <= 300:
        assert np.array_equal(S, q.astype(np.int64) @ k.astype(np.int64).T)
    targets = [g.integers(0, Nk, Nq)]
    if Nq == Nk:
        targets.insert(0, None)
    for target in targets:
        rank, best_idx, best_val, pos_val = run_rank(ops, q, k, target)
        t = np.arange(Nq) if target is None else target
        want_rank = stable_ranks(S, t)
        what = f"({Nq}, {Nk}, {D}) target={'None' if target is None else 'random'}"
        print(f"{what}: ties with the positive in {int(((S == S[np.arange(Nq), t][:, None]).sum(1) > 1).sum())} rows, "
              f"max rank {int(want_rank.max())}, rank mismatches {int((rank != want_rank).sum())}")
        assert rank.dtype == np.int32 and best_idx.dtype == np.int32
        assert np.array_equal(pos_val.astype(np.int64), S[np.arange(Nq), t]) and np.array_equal(pos_val, np.rint(pos_val)), what
        assert np.array_equal(rank.astype(np.int64), want_rank), what
        assert np.array_equal(best_idx.astype(np.int64), np.argmax(S, axis=1)), what            # np.argmax: the first maximum
        assert np.array_equal(best_val.astype(np.int64), S.max(axis=1)) and np.array_equal(best_val, np.rint(best_val)), what
        assert np.array_equal(rank == 0, np.argmax(S, axis=1) == t), what


def test_leading_dimensions_and_unaligned_rows(ops):
    """Row-major views with a leading dimension (a column slice of a wider buffer), also one that breaks 16-byte alignment."""
    g = np.random.default_rng(11)
    for Nq, Nk, D, pad, off in [(200, 333, 64, 16, 0), (200, 333, 64, 3, 1), (130, 130, 40, 8, 4)]:
        qb = g.integers(-3, 4, (Nq, D + pad)).astype(np.float32)
        kb = g.integers(-3, 4, (Nk, D + pad)).astype(np.float32)
        tq, tk = torch.from_numpy(qb).to(DEV)[:, off:off + D], torch.from_numpy(kb).to(DEV)[:, off:off + D]
        assert not tq.is_contiguous()
        target = g.integers(0, Nk, Nq)
        rank, best_idx, best_val, pos_val = [o.cpu().numpy() for o in
                                             ops.retrieval_rank(tq, tk, torch.from_numpy(target.astype(np.int32)).to(DEV))]
        S = (qb[:, off:off + D].astype(np.float64) @ kb[:, off:off + D].astype(np.float64).T).astype(np.int64)
        assert np.array_equal(rank, stable_ranks(S, target)) and np.array_equal(best_idx, np.argmax(S, 1))
        assert np.array_equal(pos_val.astype(np.int64), S[np.arange(Nq), target]) and np.array_equal(best_val.astype(np.int64), S.max(1))


# ------------------------------------------------------------------------------------------ 2. float, derived interval
def clustered_views(N, D, b):
    """Clustered unit rows: x = c[label] + 0.7 n1, q = unit(x), k = unit(x + b n2); 64 clusters; fixed seed and draw order."""
    g = np.random.default_rng(7)
    c = g.standard_normal((64, D))
    label = g.integers(0, 64, N)
    n1 = g.standard_normal((N, D))
    n2 = g.standard_normal((N, D))

    def unit(v):
        return (v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-12)).astype(np.float32)

    x = c[label] + 0.7 * n1
    return unit(x), unit(x + b * n2)


def rank_intervals(q, k, target, D):
    """Per row, the ranks an fp32 chain may report: with tau = 2 D 2^-24 (chain error <= D u sum_d |q_d k_d| <= D u for unit rows, once
    for each of the two scores compared), lo = #{S64 > pos + tau}, hi = #{S64 >= pos - tau} - 1."""
    S = q.astype(np.float64) @ k.astype(np.float64).T
    tau = 2.0 * D * 2.0 ** -24
    pos = S[np.arange(S.shape[0]), target][:, None]
    lo = (S > pos + tau).sum(1)
    hi = (S >= pos - tau).sum(1) - 1
    return S, lo, hi


FLOAT_CASES = [(4096, 384, 3.0), (2053, 1024, 3.0), (1000, 88, 1.5)]


@pytest.mark.parametrize("N,D,b", FLOAT_CASES)
def test_float_rank_within_derived_interval(ops, N, D, b):
    q, k = clustered_views(N, D, b)
    S, lo, hi = rank_intervals(q, k, np.arange(N), D)
    sharp = float((lo == hi).mean())
    rank, best_idx, best_val, pos_val = run_rank(ops, q, k)
    bad = (rank < lo) | (rank > hi)
    print(f"N={N} D={D} b={b}: one-value intervals {100 * sharp:.2f} %, top-1 {float((rank == 0).mean()):.4f}, max rank {int(rank.max())}, "
          f"rows outside their interval {int(bad.sum())}, max |pos_val - S64| {float(np.abs(pos_val - np.diagonal(S)).max()):.3e}")
    assert sharp >= 0.98, sharp                           # keeps the test sharp: nearly every row has exactly one admissible rank
    assert rank.max() > 0                                 # ... and the ranks are not all zero
    assert not bad.any(), (int(bad.sum()), np.flatnonzero(bad)[:8], rank[bad][:8], lo[bad][:8], hi[bad][:8])
    tau = 2.0 * D * 2.0 ** -24
    assert np.abs(pos_val - np.diagonal(S)).max() <= tau / 2 and np.abs(best_val - S.max(1)).max() <= tau / 2
    assert np.all(S[np.arange(N), best_idx] >= S.max(1) - tau)


# ------------------------------------------------------------------------------------------ 3. self-consistency
def test_best_idx_fed_back_is_rank_zero(ops):
    q, k = clustered_views(2053, 1024, 3.0)
    _, best_idx, best_val, _ = run_rank(ops, q, k)
    rank, best_idx2, best_val2, pos_val = run_rank(ops, q, k, best_idx)
    assert np.array_equal(rank, np.zeros_like(rank))
    assert np.array_equal(pos_val.view(np.uint32), best_val.view(np.uint32))              # bitwise the score the sweep computes
    assert np.array_equal(best_idx2, best_idx) and np.array_equal(best_val2.view(np.uint32), best_val.view(np.uint32))
    # the exact case too, where many keys share the maximum
    g = np.random.default_rng(5)
    qi, ki = g.integers(-3, 4, (515, 96)).astype(np.float32), g.integers(-3, 4, (901, 96)).astype(np.float32)
    _, bi, bv, _ = run_rank(ops, qi, ki, g.integers(0, 901, 515))
    rank, _, _, pv = run_rank(ops, qi, ki, bi)
    assert not rank.any() and np.array_equal(pv.view(np.uint32), bv.view(np.uint32))


def test_duplicated_keys_tie_and_lower_index_wins(ops):
    q, k = clustered_views(1000, 88, 1.5)
    k = k.copy()
    k[500:] = k[:500]                                     # key 500 + i is bitwise key i
    t_lo = np.random.default_rng(3).integers(0, 500, 1000)
    rank_lo, best_idx, best_val, pos_lo = run_rank(ops, q, k, t_lo)
    rank_hi, best_idx_hi, best_val_hi, pos_hi = run_rank(ops, q, k, t_lo + 500)
    assert np.array_equal(pos_lo.view(np.uint32), pos_hi.view(np.uint32))                 # equal rows, equal scores
    # rank_hi - rank_lo = #{t <= j < t + 500 : s(i,j) == pos}: the twin with the lower index is placed first, so it is at least 1;
    # anything more is an accidental bitwise tie between different keys (about 1e-7 per pair)
    assert np.all(rank_hi >= rank_lo + 1) and (rank_hi == rank_lo + 1).mean() >= 0.99
    assert best_idx.max() < 500 and np.array_equal(best_idx, best_idx_hi)                 # ... and it wins the maximum
    assert np.array_equal(best_val.view(np.uint32), best_val_hi.view(np.uint32))
    _, lo, hi = rank_intervals(q, k, t_lo, 88)
    assert np.all((rank_lo >= lo) & (rank_lo <= hi))


def test_two_runs_are_bit_identical(ops):
    q, k = clustered_views(4096, 384, 3.0)
    for x, y in zip(run_rank(ops, q, k), run_rank(ops, q, k)):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    t = np.random.default_rng(9).integers(0, 4096, 4096)
    for x, y in zip(run_rank(ops, q, k, t), run_rank(ops, q, k, t)):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


def test_argument_errors(ops):
    z = torch.zeros(4, 8, device=DEV)
    with pytest.raises(ValueError, match="Nq must equal Nk"):
        ops.retrieval_rank(z, torch.zeros(5, 8, device=DEV))
    with pytest.raises(ValueError, match="fp32"):
        ops.retrieval_rank(z.bfloat16(), z.bfloat16())
    with pytest.raises(ValueError, match="target must have shape"):
        ops.retrieval_rank(z, z, torch.zeros(3, dtype=torch.int32, device=DEV))
    for bad in (torch.tensor([0, 1, 2, 4], device=DEV), torch.tensor([0, -1, 2, 3], device=DEV), torch.tensor([0, 1, 2, 2 ** 32], device=DEV)):
        with pytest.raises(ValueError, match="target indices must lie in"):
            ops.retrieval_rank(z, z, bad)
    with pytest.raises(ValueError, match="int32 or int64"):
        ops.retrieval_rank(z, z, torch.zeros(4, device=DEV))
    assert ops.retrieval_rank(z, z, torch.tensor([3, 2, 1, 0], device=DEV))[0].tolist() == [3, 2, 1, 0]      # int64 indices; all scores tie


# ------------------------------------------------------------------------------------------ 4. end to end
TINY = dict(img_size=56, patch=14, dim=64, depth=2, heads=2, num_registers=4, scale_aware=True)


def tiny_student():
    import zoo.arch as arch
    from oracle import dinox_oracle as O
    cfg = O.VitCfg(out_dim=256, **TINY)
    sd = O.random_params(cfg, seed=1)
    student = arch.DinoStudentTeacher(arch.PatchViT(**TINY), 256)
    student.load_state_dict(sd)
    return student.to(DEV).eval(), sd, cfg


def test_embed_cls_matches_oracle(ops):
    from dinox import retrieval
    from oracle import dinox_oracle as O
    student, sd, cfg = tiny_student()
    g = torch.Generator().manual_seed(2)
    x = torch.randn(8, 3, 56, 56, generator=g)
    sp = torch.rand(8, 3, generator=g) * 2 + 0.4
    got = retrieval.embed_cls(student.backbone, x.to(DEV), sp.to(DEV))
    assert got.dtype == torch.float32 and got.shape == (8, 64) and got.is_cuda
    with torch.no_grad():
        feats = O.vit_forward(sd, x, sp, cfg, pre="backbone.")
    want = torch.nn.functional.normalize(feats[:, 0].float(), p=2, dim=-1)
    err = (got.cpu().double() - want.double()).abs().max().item()
    print(f"embed_cls vs oracle: max abs err {err:.3e} (scale {want.abs().max().item():.3e})")
    assert err <= 1e-3 * want.abs().max().item()
    assert torch.allclose(got.norm(dim=-1).cpu(), torch.ones(8), atol=1e-6)


def test_view_retrieval_metrics_match_float64_ranking(ops, cli):
    from dinox import retrieval
    student, _, _ = tiny_student()
    n = 96
    ds = cli.SyntheticSliceDataset(n, img_size=56, seed=3)
    idxs = random.Random(0).sample(range(n), k=n)

    def seed():
        random.seed(0)
        np.random.seed(0)
        torch.manual_seed(0)

    seed()
    res = retrieval.view_retrieval(student, ds, idxs, batch_size=40, scale_aware=True, topk=5, ratio=10.0)
    assert set(res) == {"top1", "topk_acc", "random_baseline", "ratio_vs_random", "passed", "embedding_std_mean", "embedding_norm_mean"}
    # the same views again (same seeds), this time keeping the embeddings: rank them in float64 on the host
    seed()
    Q, K, stats = retrieval.embed_views(student, ds, idxs, batch_size=40, scale_aware=True)
    rank = ops.retrieval_rank(Q, K)[0].cpu().numpy()
    q, k = Q.cpu().numpy(), K.cpu().numpy()
    assert q.shape == (n, 64) and k.shape == (n, 64) and Q.is_cuda
    assert np.allclose(np.linalg.norm(q, axis=1), 1.0, atol=1e-6)
    _, lo, hi = rank_intervals(q, k, np.arange(n), 64)
    assert np.all((rank >= lo) & (rank <= hi))
    wide = int((lo != hi).sum())
    m_lo, m_hi = retrieval.metrics_from_ranks(lo, 5, 10.0), retrieval.metrics_from_ranks(hi, 5, 10.0)
    print(f"view_retrieval: {res}; rows with a wider interval: {wide}")
    assert {key: res[key] for key in m_lo} == retrieval.metrics_from_ranks(rank, 5, 10.0)        # deterministic: same seeds, same ranks
    for key in ("top1", "topk_acc", "ratio_vs_random"):
        assert m_hi[key] <= res[key] <= m_lo[key], key
    if wide == 0:
        assert {key: res[key] for key in m_lo} == m_lo
    assert res["random_baseline"] == 1.0 / n
    assert stats == {key: res[key] for key in stats} and res["embedding_std_mean"] > 0.0 and res["embedding_norm_mean"] > 0.0
    # the bf16 backbone runs too and keeps fp32 unit rows
    seed()
    Qa, _, sa = retrieval.embed_views(student, ds, idxs, batch_size=40, scale_aware=True, amp_dtype=torch.bfloat16)
    assert Qa.dtype == torch.float32 and abs(sa["embedding_norm_mean"] - res["embedding_norm_mean"]) < 0.05 * res["embedding_norm_mean"]


def test_embedding_statistics_from_running_sums(ops, cli):
    """embedding_std_mean / embedding_norm_mean against torch's own std / norm on the un-normalised rows, on a dataset whose two
    views are fixed tensors (so a second pass sees the same inputs)."""
    from dinox import retrieval
    student, _, _ = tiny_student()
    g = torch.Generator().manual_seed(4)
    items = [([torch.randn(3, 56, 56, generator=g), torch.randn(3, 56, 56, generator=g)], torch.rand(3, generator=g) + 0.5) for _ in range(50)]
    _, _, stats = retrieval.embed_views(student, items, list(range(50)), batch_size=16, scale_aware=True)
    raw = retrieval._cls_rows(student.backbone, torch.stack([v[0] for v, _ in items]).to(DEV), torch.stack([s for _, s in items]).to(DEV)).cpu()
    assert abs(stats["embedding_std_mean"] - float(raw.std(dim=0).mean())) <= 1e-4 * float(raw.std(dim=0).mean())
    assert abs(stats["embedding_norm_mean"] - float(raw.norm(dim=-1).mean())) <= 1e-4 * float(raw.norm(dim=-1).mean())


def test_non_finite_embeddings_do_not_pass_the_gate(ops):
    """Every comparison with a NaN score is false: the kernel reports rank 0 for such rows (documented), so the evaluation must refuse."""
    from dinox import retrieval
    student, _, _ = tiny_student()
    g = torch.Generator().manual_seed(6)
    items = [([torch.randn(3, 56, 56, generator=g), torch.randn(3, 56, 56, generator=g)], torch.ones(3)) for _ in range(8)]
    items[3][0][0][0, 0, 0] = float("nan")
    with pytest.raises(FloatingPointError, match="non-finite"):
        retrieval.view_retrieval(student, items, list(range(8)), batch_size=4, scale_aware=True)
    q = torch.randn(5, 16, device=DEV)
    q[2] = float("nan")
    rank, best_idx, best_val, pos_val = ops.retrieval_rank(q, torch.randn(5, 16, device=DEV))
    assert torch.isnan(pos_val[2]) and torch.isfinite(pos_val[[0, 1, 3, 4]]).all() and int(rank[2]) == 0


REFERENCE_JSON_KEYS = {"kind", "version", "created_at", "checkpoint", "step", "index_csv", "split_manifest", "img_size", "n", "seed",
                       "batch_size", "topk", "top1", "topk_acc", "random_baseline", "ratio_vs_random", "pass_ratio", "passed", "seconds",
                       "model"}


@pytest.mark.parametrize("ckpt_name", ["ref_checkpoint_00000003.pth", "engine_checkpoint_00000003.pth"])
def test_script_on_checkpoint(tmp_path, ckpt_name):
    """The drop-in script on a reference-written (and an engine-written) checkpoint: scale-aware 28 px, patch 14, width 32, so the
    rank kernel runs at D = 32."""
    ckpt = tmp_path / ckpt_name
    shutil.copy(os.path.join(GOLDEN, ckpt_name), ckpt)
    script = os.path.join(ROOT, "dino-x_amd", "scripts", "phase5_view_retrieval_eval.py")
    p = subprocess.run([sys.executable, script, "--checkpoint", str(ckpt), "--synthetic", "64", "--scale-aware"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    print(p.stdout)
    print(p.stderr[-2000:])
    assert p.returncode in (0, 2), p.stderr[-2000:]
    out = tmp_path / "view_retrieval_step3_N64.json"                   # --n 4096 capped to the 64 rows there are
    assert out.exists()
    m = json.loads(out.read_text())
    assert set(m) == REFERENCE_JSON_KEYS | {"embedding_std_mean", "embedding_norm_mean"}
    assert set(m["model"]) == {"name", "patch", "dim", "depth", "heads", "mlp_ratio", "out_dim", "ln_out_dim"}
    assert m["kind"] == "phase5_view_retrieval" and m["version"] == 1 and m["n"] == 64 and m["step"] == 3 and m["img_size"] == 28
    assert m["model"]["dim"] == 32 and m["topk"] == 5 and m["pass_ratio"] == 10.0 and m["random_baseline"] == 1.0 / 64
    assert abs(m["top1"] * 64 - round(m["top1"] * 64)) < 1e-9 and abs(m["topk_acc"] * 64 - round(m["topk_acc"] * 64)) < 1e-9
    assert 0.0 <= m["top1"] <= m["topk_acc"] <= 1.0
    assert m["passed"] == (m["top1"] >= 10.0 / 64) and p.returncode == (0 if m["passed"] else 2)
    lines = [ln for ln in p.stdout.splitlines() if "=" in ln and not ln.startswith("⚠")]
    assert lines[-4] == "ok=true" and lines[-3] == f"passed={str(m['passed']).lower()}"
    assert lines[-2].startswith(f"top1={m['top1']:.6f} top5={m['topk_acc']:.6f} baseline={1.0 / 64:.6f} ratio=")
    assert lines[-1] == f"metrics_json={out}"
