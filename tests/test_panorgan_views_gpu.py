"""GPU tests of the windowed similarity-rank kernel and the paired row dots (csrc/retrieval.hip: dinox_retrieval_rank_windowed,
dinox_row_dots) and of the two pan-organ metrics built on them (dinox/retrieval.py: view_retrieval_per_dataset, spacing_counterfactual;
scripts/evaluate_panorgan.py --view-metrics).  Run with ``-m gpu`` on an MI355X.

Shapes: seven groups of (1, 31, 130, 257, 5, 128, 300) rows, 852 in all -- a group of one, one below a wave's 32 rows, groups that
straddle the 128-row strip and tile boundaries, a strip holding more than two groups, one exactly tile-sized group at an unaligned
offset -- at D = 7 (element loads), 88 (no multiple of 16) and 384 (the real width).

1. exact case: integer rows in {-3..3}, every score exact in fp32, outputs EQUAL a NumPy restatement of the windowed semantics;
2. float case: bitwise agreement with group-by-group calls of the unwindowed kernel, and the float64 interval of each rank;
3. row_dots bitwise against retrieval_rank's pos_val; determinism; argument errors;
4. the metrics: against the recorded reference results (tests/golden/panorgan_views.npz), against per-group view_retrieval, against
   the CPU oracle, and the script end to end.
"""
import importlib.util
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
GROUPS = (1, 31, 130, 257, 5, 128, 300)
N = sum(GROUPS)
DIMS = (7, 88, 384)
EMPTY_IDX = 0x7fffffff
SCRIPT = os.path.join(ROOT, "dino-x_amd", "scripts", "evaluate_panorgan.py")


@pytest.fixture(scope="module")
def ops():
    from dinox import ops
    import dinox._lib as L
    assert L.lib.dinox_device_ok() == 1, L.last_error()
    return ops


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def host(out):
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]                 # rank, best_idx, best_val, pos_val


def group_windows(groups=GROUPS):
    hi = np.cumsum(groups)
    return np.repeat(hi - np.asarray(groups), groups), np.repeat(hi, groups)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def windowed_reference(S, target, lo, hi):
    """The windowed semantics of include/dinox.h on a host score matrix: bounds clamped into [0, Nk]; rank counts window keys only;
    best_* is the window's maximum and its lowest (global) index, (0x7fffffff, -inf) for an empty window."""
    Nq, Nk = S.shape
    lo, hi = np.clip(lo, 0, Nk), np.clip(hi, 0, Nk)
    j = np.arange(Nk)[None, :]
    inside = (j >= lo[:, None]) & (j < hi[:, None])
    pos = S[np.arange(Nq), target]
    ahead = (S > pos[:, None]) | ((S == pos[:, None]) & (j < target[:, None]))
    rank = (ahead & inside).sum(1)
    masked = np.where(inside, S.astype(np.float64), -np.inf)
    empty = ~inside.any(1)
    best_idx = np.where(empty, EMPTY_IDX, masked.argmax(1))                # np.argmax: the first maximum
    return rank, best_idx, masked.max(1), pos


def integer_rows(Nq, Nk, D):
    g = np.random.default_rng(Nq * 7 + Nk * 3 + D)
    q = g.integers(-3, 4, (Nq, D)).astype(np.float32)
    k = g.integers(-3, 4, (Nk, D)).astype(np.float32)
    S = (q.astype(np.float64) @ k.astype(np.float64).T).astype(np.int64)  # |s| <= 9 D < 2^14: exact
    return g, q, k, S


def check_exact(got, want, what):
    rank, best_idx, best_val, pos_val = got
    w_rank, w_idx, w_val, w_pos = want
    assert rank.dtype == np.int32 and best_idx.dtype == np.int32
    assert np.array_equal(pos_val.astype(np.float64), w_pos.astype(np.float64)), what
    assert np.array_equal(rank.astype(np.int64), w_rank), (what, np.flatnonzero(rank != w_rank)[:8])
    assert np.array_equal(best_idx.astype(np.int64), w_idx), (what, np.flatnonzero(best_idx != w_idx)[:8])
    assert np.array_equal(best_val.astype(np.float64), w_val), what


# ------------------------------------------------------------------------------------------ 1. exact
@pytest.mark.parametrize("D", DIMS)
def test_exact_integer_scores_in_group_windows(ops, D):
    g, q, k, S = integer_rows(N, N, D)
    lo, hi = group_windows()
    in_window = (lo + g.integers(0, 1 << 30, N) % (hi - lo)).astype(np.int64)
    for target in (None, in_window):
        got = host(ops.retrieval_rank_windowed(dev(q), dev(k), dev(lo, torch.int32), dev(hi, torch.int32),
                                               None if target is None else dev(target, torch.int32)))
        t = np.arange(N) if target is None else target
        want = windowed_reference(S, t, lo, hi)
        what = f"D={D} target={'None' if target is None else 'in-window'}"
        j = np.arange(N)[None, :]
        ties = ((S == want[3][:, None]) & (j >= lo[:, None]) & (j < hi[:, None])).sum(1)
        print(f"{what}: ties with the positive inside the window in {int((ties > 1).sum())} rows, max rank {int(want[0].max())}")
        check_exact(got, want, what)
        assert np.all((got[1] >= lo) & (got[1] < hi))                      # a global key index inside the window
        assert int(got[0][0]) == 0 and int(got[1][0]) == 0                 # the group of one


def test_exact_integer_scores_in_arbitrary_windows(ops):
    """Unsorted windows with gaps between them, empty and inverted windows, bounds outside [0, Nk] (clamped, never an address), targets
    outside their window, more queries than keys."""
    Nq, Nk, D = 852, 700, 88
    g, q, k, S = integer_rows(Nq, Nk, D)
    lo = g.integers(-60, Nk + 40, Nq).astype(np.int64)
    hi = lo + g.integers(0, 400, Nq)
    target = g.integers(0, Nk, Nq).astype(np.int64)
    lo[0], hi[0] = 10, 10                                                  # empty
    lo[1], hi[1] = 500, 100                                                # inverted: empty
    lo[2], hi[2], target[2] = 650, 5000, 3                                 # clamped at Nk, target outside
    lo[3], hi[3], target[3] = -7, 40, 699                                  # clamped at 0, target outside
    lo[4], hi[4] = 2 ** 40, 2 ** 41                                        # far outside: empty after clamping
    lo[5], hi[5] = -2 ** 40, 2 ** 40                                       # every key
    lo[128:256], hi[128:256] = 0, 0                                        # a whole strip without a window
    lo[300:310], hi[300:310] = 0, 5                                        # a hull with a gap: keys [0, 5) and ...
    lo[310:320], hi[310:320] = 690, 700                                    # ... [690, 700) in one strip
    want = windowed_reference(S, target, lo, hi)
    empty = np.clip(lo, 0, Nk) >= np.clip(hi, 0, Nk)
    outside = (target < lo) | (target >= hi)
    assert empty[[0, 1, 4]].all() and empty.sum() > 130 and (outside & ~empty).sum() > 100
    got = host(ops.retrieval_rank_windowed(dev(q), dev(k), dev(lo), dev(hi), dev(target)))             # int64 indices
    check_exact(got, want, "arbitrary windows")
    assert not got[0][empty].any() and np.all(got[1][empty] == EMPTY_IDX) and np.all(np.isneginf(got[2][empty]))
    assert np.array_equal(got[3][empty].astype(np.int64), S[np.arange(Nq), target][empty])              # pos_val is still written
    # int32 bounds that need the kernel's own clamp
    lo32, hi32 = np.clip(lo, -2 ** 31, 2 ** 31 - 1).astype(np.int32), np.clip(hi, -2 ** 31, 2 ** 31 - 1).astype(np.int32)
    check_exact(host(ops.retrieval_rank_windowed(dev(q), dev(k), dev(lo32), dev(hi32), dev(target, torch.int32))), want, "int32 bounds")


# ------------------------------------------------------------------------------------------ 2. float: bitwise against the unwindowed kernel
FLOAT_SEED = 7
FLOAT_B = {7: 1.5, 88: 4.0, 384: 8.0}          # view noise per width: top-1 well inside (0, 1) in groups of a few hundred rows


def clustered_views(n, D, b, seed=FLOAT_SEED):
    """Clustered unit rows (the generator of tests/test_retrieval_gpu.py): x = c[label] + 0.7 n1, q = unit(x), k = unit(x + b n2)."""
    g = np.random.default_rng(seed)
    c = g.standard_normal((64, D))
    label = g.integers(0, 64, n)
    n1 = g.standard_normal((n, D))
    n2 = g.standard_normal((n, D))

    def unit(v):
        return (v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-12)).astype(np.float32)

    x = c[label] + 0.7 * n1
    return unit(x), unit(x + b * n2)


def rank_intervals(q, k, target, D):
    """Per row, the ranks an fp32 chain may report (tests/test_retrieval_gpu.py): tau = 2 D 2^-24, lo = #{S64 > pos + tau},
    hi = #{S64 >= pos - tau} - 1."""
    S = q.astype(np.float64) @ k.astype(np.float64).T
    tau = 2.0 * D * 2.0 ** -24
    pos = S[np.arange(S.shape[0]), target][:, None]
    return (S > pos + tau).sum(1), (S >= pos - tau).sum(1) - 1


def group_intervals(q, k, D, groups=GROUPS):
    lo, hi, at = [], [], 0
    for n in groups:
        a, b = rank_intervals(q[at:at + n], k[at:at + n], np.arange(n), D)
        lo.append(a)
        hi.append(b)
        at += n
    return np.concatenate(lo), np.concatenate(hi)


@pytest.mark.parametrize("D", DIMS)
def test_bitwise_equal_to_the_unwindowed_kernel_per_group(ops, D):
    q, k = clustered_views(N, D, FLOAT_B[D])
    tq, tk = dev(q), dev(k)
    lo, hi = group_windows()
    rank, best_idx, best_val, pos_val = host(ops.retrieval_rank_windowed(tq, tk, dev(lo, torch.int32), dev(hi, torch.int32)))
    at = 0
    for n in GROUPS:
        r, bi, bv, pv = host(ops.retrieval_rank(tq[at:at + n], tk[at:at + n]))
        sl = slice(at, at + n)
        assert np.array_equal(rank[sl], r), (D, n)
        assert np.array_equal(bits(pos_val[sl]), bits(pv)) and np.array_equal(bits(best_val[sl]), bits(bv)), (D, n)
        assert np.array_equal(best_idx[sl], bi + at), (D, n)
        at += n
    r_lo, r_hi = group_intervals(q, k, D)
    sharp = float((r_lo == r_hi).mean())
    bad = (rank < r_lo) | (rank > r_hi)
    print(f"D={D}: one-value intervals {100 * sharp:.2f} %, top-1 {float((rank == 0).mean()):.4f}, max rank {int(rank.max())}, "
          f"rows outside their interval {int(bad.sum())}")
    assert sharp >= 0.98, sharp
    assert rank.max() > 0 and not bad.any(), (int(bad.sum()), np.flatnonzero(bad)[:8])
    # every window = every key: the unwindowed entry, bit for bit
    full = host(ops.retrieval_rank_windowed(tq, tk, dev(np.zeros(N, np.int32)), dev(np.full(N, N, np.int32))))
    for x, y in zip(full, host(ops.retrieval_rank(tq, tk))):
        assert np.array_equal(bits(x), bits(y)), D


# ------------------------------------------------------------------------------------------ 3. row_dots, determinism, errors
@pytest.mark.parametrize("n", [1, 33, 300])
@pytest.mark.parametrize("D", [7, 384])
def test_row_dots_is_the_pos_val_of_retrieval_rank(ops, n, D):
    a, b = clustered_views(n, D, FLOAT_B[D], seed=n + D)
    ta, tb = dev(a), dev(b)
    out = ops.row_dots(ta, tb)
    assert out.dtype == torch.float32 and out.shape == (n,) and out.is_cuda
    out = out.cpu().numpy()
    assert np.array_equal(bits(out), bits(ops.retrieval_rank(ta, tb)[3].cpu().numpy()))
    exact = (a.astype(np.float64) * b.astype(np.float64)).sum(1)
    print(f"n={n} D={D}: max |row_dots - float64| {np.abs(out - exact).max():.3e} (bound {D * 2.0 ** -24:.3e})")
    assert np.abs(out - exact).max() <= D * 2.0 ** -24                      # chain error <= D u sum |a_d b_d| <= D u for unit rows
    if n == 300:                                                            # column slices of wider buffers: a leading dimension,
        wa, wb = torch.randn(n, D + 9, device=DEV), torch.randn(n, D + 5, device=DEV)      # one of them off 16-byte alignment
        wa[:, 1:1 + D], wb[:, 4:4 + D] = ta, tb
        va, vb = wa[:, 1:1 + D], wb[:, 4:4 + D]
        assert not va.is_contiguous() and not vb.is_contiguous()
        assert np.array_equal(bits(ops.row_dots(va, vb).cpu().numpy()), bits(out))


def test_two_runs_are_bit_identical(ops):
    q, k = clustered_views(N, 384, FLOAT_B[384])
    lo, hi = group_windows()
    args = (dev(q), dev(k), dev(lo, torch.int32), dev(hi, torch.int32))
    t = dev(np.random.default_rng(9).integers(0, N, N), torch.int32)
    for target in (None, t):
        for x, y in zip(host(ops.retrieval_rank_windowed(*args, target)), host(ops.retrieval_rank_windowed(*args, target))):
            assert np.array_equal(bits(x), bits(y))
    assert np.array_equal(bits(ops.row_dots(args[0], args[1]).cpu().numpy()), bits(ops.row_dots(args[0], args[1]).cpu().numpy()))


def test_argument_errors(ops):
    z, w = torch.zeros(4, 8, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV)
    full = torch.full((4,), 4, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="Nq must equal Nk"):
        ops.retrieval_rank_windowed(z, torch.zeros(5, 8, device=DEV), w, full)
    with pytest.raises(ValueError, match="fp32"):
        ops.retrieval_rank_windowed(z.bfloat16(), z.bfloat16(), w, full)
    with pytest.raises(ValueError, match="key_lo must have shape"):
        ops.retrieval_rank_windowed(z, z, w[:3], full)
    with pytest.raises(ValueError, match="key_hi must be int32 or int64"):
        ops.retrieval_rank_windowed(z, z, w, full.float())
    with pytest.raises(ValueError, match="target must have shape"):
        ops.retrieval_rank_windowed(z, z, w, full, torch.zeros(3, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="int32 or int64"):
        ops.retrieval_rank_windowed(z, z, w, full, torch.zeros(4, device=DEV))
    for bad in (torch.tensor([0, 1, 2, 4], device=DEV), torch.tensor([0, -1, 2, 3], device=DEV), torch.tensor([0, 1, 2, 2 ** 32], device=DEV)):
        with pytest.raises(ValueError, match="target indices must lie in"):
            ops.retrieval_rank_windowed(z, z, w, full, bad)
    # window bounds outside [0, Nk] are no error; all scores tie, so the rank is the number of window keys below the target
    rank = ops.retrieval_rank_windowed(z, z, torch.tensor([-5, 0, 1, 2], device=DEV), torch.tensor([99, 4, 4, 3], device=DEV),
                                       torch.tensor([3, 2, 1, 0], device=DEV))[0]
    assert rank.tolist() == [3, 2, 0, 0]
    with pytest.raises(ValueError, match="fp32"):
        ops.row_dots(z.double(), z.double())
    with pytest.raises(ValueError, match="shapes must be equal"):
        ops.row_dots(z, torch.zeros(5, 8, device=DEV))
    with pytest.raises(ValueError, match="empty operand"):
        ops.row_dots(z[:0], z[:0])


# ------------------------------------------------------------------------------------------ 4. the metrics
TINY = dict(img_size=56, patch=14, dim=64, depth=2, heads=2, num_registers=4, scale_aware=True)
SCALE_OUT_GAIN = 1.0                    # on scale_embed's output layer: see counterfactual_params


def counterfactual_params():
    """The oracle's seeded parameters (seed 1, as tests/test_retrieval_gpu.py).  Checked on the CPU when this test was written: with them
    the oracle's unit CLS rows at spacing, 2 x and 0.5 x differ pairwise by 0.12 or more in max-abs over a batch of 8 random images, against a gate
    of 1e-3 max|e| = 3.6e-4 -- so the seeded output layer of scale_embed needs no gain."""
    from oracle import dinox_oracle as O
    cfg = O.VitCfg(out_dim=256, **TINY)
    sd = O.random_params(cfg, seed=1)
    sd["backbone.scale_embed.mlp.2.weight"] = sd["backbone.scale_embed.mlp.2.weight"] * SCALE_OUT_GAIN
    return sd, cfg


def tiny_student(scale_aware=True):
    import zoo.arch as arch
    sd, cfg = counterfactual_params()
    kw = dict(TINY, scale_aware=scale_aware)
    student = arch.DinoStudentTeacher(arch.PatchViT(**kw), 256)
    student.load_state_dict({k: v for k, v in sd.items() if scale_aware or "scale_embed" not in k})
    return student.to(DEV).eval(), sd, cfg


@pytest.fixture(scope="module")
def script():
    spec = importlib.util.spec_from_file_location("evaluate_panorgan_views_gpu", SCRIPT)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def seed_all(s=0):
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


def test_recorded_reference_embeddings_give_the_reference_result(ops):
    """The reference's own Q and K rows (its PatchViT on the CPU) through the windowed kernel: its result dict, exactly -- the fixture has
    no key within 2 D 2^-23 of a positive, so every rank has one admissible value."""
    from dinox import retrieval
    z = np.load(os.path.join(GOLDEN, "panorgan_views.npz"))
    names = [str(n) for n in z["names"]]
    want = json.loads(str(z["reference_retrieval"]))
    Q = dev(np.concatenate([z[f"Q_{g}"] for g in range(len(names))]))
    K = dev(np.concatenate([z[f"K_{g}"] for g in range(len(names))]))
    sizes = [z[f"Q_{g}"].shape[0] for g in range(len(names))]
    got = retrieval.per_dataset_retrieval_from_embeddings(Q, K, sizes, names, topk=int(z["topk"]))
    assert list(got) == list(want)
    for name in want:
        assert list(got[name]) == list(want[name])
        for key, w in want[name].items():
            assert abs(got[name][key] - w) <= 1e-12, (name, key, got[name][key], w)
    # through view_retrieval_per_dataset itself, with embed_views replaced by the recorded rows of the picks it asks for
    labels = [str(d) for d in z["datasets"]]
    rows_of = {name: [i for i, d in enumerate(labels) if d == name] for name in names}
    row_q, row_k = {}, {}
    for g, name in enumerate(names):
        for j, p in enumerate(z[f"picks_{g}"]):
            row_q[rows_of[name][p]], row_k[rows_of[name][p]] = z[f"Q_{g}"][j], z[f"K_{g}"][j]

    def recorded(student, dataset, idxs, batch_size=64, scale_aware=False, *, amp_dtype=None):
        return dev(np.stack([row_q[i] for i in idxs])), dev(np.stack([row_k[i] for i in idxs])), {}

    real, retrieval.embed_views = retrieval.embed_views, recorded
    try:
        got2 = retrieval.view_retrieval_per_dataset(None, labels, labels, n_per_dataset=int(z["n_per_dataset"]), seed=int(z["seed"]),
                                                    topk=int(z["topk"]))
    finally:
        retrieval.embed_views = real
    assert got2 == got


def test_view_retrieval_per_dataset_equals_per_group_view_retrieval(ops, cli, script):
    from dinox import retrieval
    student, _, _ = tiny_student()
    n = 56
    ds = cli.SyntheticSliceDataset(n, img_size=56, seed=3)
    labels = [script.synthetic_label(i) for i in range(n)]                  # 32 / 16 / 8 rows
    kw = dict(batch_size=4, scale_aware=True)                               # every group a whole number of batches: equal launches
    seed_all()
    got = retrieval.view_retrieval_per_dataset(student, ds, labels, n_per_dataset=12, seed=5, topk=5, **kw)
    names, picks = retrieval.per_dataset_picks(labels, 12, 5)
    assert list(got) == names == sorted(set(labels)) and [got[m]["n"] for m in names] == [12, 12, 8]
    seed_all()                                                              # the same draws: dataset by dataset, item by item
    for name, p in zip(names, picks):
        assert all(labels[i] == name for i in p) and len(set(p)) == len(p)
        one = retrieval.view_retrieval(student, ds, p, topk=5, **kw)
        print(name, got[name], one)
        assert list(got[name]) == ["n", "top1", "top5", "random_baseline", "ratio_vs_random"]
        assert got[name]["top1"] == one["top1"] and got[name]["top5"] == one["topk_acc"]
        assert got[name]["random_baseline"] == one["random_baseline"] == 1.0 / len(p)
        assert got[name]["ratio_vs_random"] == one["ratio_vs_random"]
    with pytest.raises(ValueError, match="labels"):
        retrieval.view_retrieval_per_dataset(student, ds, labels[:-1], **kw)
    # a NaN input must not pass as "every positive first"
    g = torch.Generator().manual_seed(6)
    items = [([torch.randn(3, 56, 56, generator=g), torch.randn(3, 56, 56, generator=g)], torch.ones(3)) for _ in range(8)]
    items[3][0][0][0, 0, 0] = float("nan")
    with pytest.raises(FloatingPointError, match="non-finite"):
        retrieval.view_retrieval_per_dataset(student, items, ["a", "b"] * 4, n_per_dataset=4, **kw)


def test_spacing_counterfactual_against_oracle_and_float64(ops, cli):
    from dinox import retrieval
    from dinox.views import make_views
    from oracle import dinox_oracle as O
    student, sd, cfg = tiny_student()
    n, D = 40, 64
    ds = cli.SyntheticSliceDataset(n, img_size=56, seed=3)
    ds.raw_views = True
    idxs = random.Random(42).sample(range(n), k=24)
    e = retrieval.embed_spacing_variants(student, ds, idxs, 56, batch_size=16)
    assert all(x.shape == (24, D) and x.dtype == torch.float32 and x.is_cuda for x in e)
    # the first batch against the CPU oracle at spacing, 2 x spacing, 0.5 x spacing
    batch = next(retrieval._eval_batches(ds, idxs[:16], 16, torch.device(DEV)))
    x, sp = make_views(batch, 56).float().cpu(), batch.spacing.cpu()
    want = []
    with torch.no_grad():
        for mult in (1.0, 2.0, 0.5):
            feats = O.vit_forward(sd, x, sp * mult, cfg, pre="backbone.")
            want.append(torch.nn.functional.normalize(feats[:, 0].float(), p=2, dim=-1).double())
    gate = 1e-3 * max(w.abs().max().item() for w in want)
    for got, w, what in zip(e, want, ("real", "2x", "half")):
        err = (got[:16].cpu().double() - w).abs().max().item()
        print(f"{what}: max abs err vs oracle {err:.3e} (gate {gate:.3e})")
        assert err <= gate, what
    for a, b, what in ((0, 1, "real vs 2x"), (0, 2, "real vs half"), (2, 1, "half vs 2x")):
        apart = (want[a] - want[b]).abs().max().item()
        print(f"oracle {what}: max abs difference {apart:.3e}")
        assert apart >= 10 * gate, what                                    # a swapped or missing multiplier cannot pass the gate
    # distances: float64 1 - a . b of the device's own unit rows
    d = retrieval.counterfactual_distances(*e)
    h = [x.cpu().numpy().astype(np.float64) for x in e]
    for got, (a, b) in zip(d, ((0, 1), (0, 2), (2, 1))):
        exact = 1.0 - (h[a] * h[b]).sum(1)
        assert got.shape == (24,) and np.abs(got - exact).max() <= (D + 2) * 2.0 ** -24
        assert got.mean() > 1e-3
    res = retrieval.spacing_counterfactual(student, ds, 56, n=24, seed=42, batch_size=16)
    assert res == retrieval.counterfactual_summary(*d) and res["n"] == 24
    assert retrieval.spacing_counterfactual(student, ds, 56, n=1000, seed=42, batch_size=16)["n"] == n      # capped at the rows there are
    plain, _, _ = tiny_student(scale_aware=False)
    assert retrieval.spacing_counterfactual(plain, ds, 56, n=24) == {"skipped": True, "reason": "baseline model has no scale embedding"}


EXISTING_KEYS = ["domain_clustering", "knn_probe", "dataset_discrimination_probe", "spacing_prediction", "embedding_stats"]


def test_script_with_view_metrics(tmp_path):
    ckpt = tmp_path / "ref_checkpoint_00000003.pth"
    shutil.copy(os.path.join(GOLDEN, "ref_checkpoint_00000003.pth"), ckpt)
    base = [sys.executable, SCRIPT, "--checkpoint", str(ckpt), "--synthetic", "64", "--scale-aware", "--probes"]
    runs = {}
    for tag, extra in (("views", ["--view-metrics"]), ("plain", []), ("skip", ["--view-metrics", "--skip-view-retrieval"])):
        out = tmp_path / f"eval_{tag}.json"
        p = subprocess.run(base + ["--out", str(out)] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        print(p.stdout)
        print(p.stderr[-2000:])
        assert p.returncode == 0, p.stderr[-2000:]
        assert p.stdout.splitlines()[-1] == "ok=true"
        runs[tag] = (json.loads(out.read_text()), p.stdout)
    m, stdout = runs["views"]
    D = m["model"]["dim"]
    assert list(m["metrics"]) == EXISTING_KEYS + ["view_retrieval_per_dataset", "spacing_counterfactual"]
    vr, cf = m["metrics"]["view_retrieval_per_dataset"], m["metrics"]["spacing_counterfactual"]
    assert list(vr) == m["datasets"] and sum(d["n"] for d in vr.values()) == 64
    for name, d in vr.items():
        assert list(d) == ["n", "top1", "top5", "random_baseline", "ratio_vs_random"]
        assert abs(d["top1"] * d["n"] - round(d["top1"] * d["n"])) < 1e-9 and 0.0 <= d["top1"] <= d["top5"] <= 1.0
        assert f"  {name}: top1={d['top1']:.4f} ratio={d['ratio_vs_random']:.1f}×" in stdout.splitlines()
    assert cf["n"] == 64 and list(cf)[0] == "n" and list(cf)[-1] == "interpretation"
    for key in ("cosine_distance_real_vs_2x", "cosine_distance_real_vs_half", "cosine_distance_half_vs_2x"):
        assert list(cf[key]) == ["mean", "std", "median"]
        assert np.isfinite(cf[key]["mean"]) and cf[key]["mean"] >= -(D + 2) * 2.0 ** -24
    assert f"  real→2x: dist={cf['cosine_distance_real_vs_2x']['mean']:.4f}" in stdout.splitlines()
    assert f"  real→½x: dist={cf['cosine_distance_real_vs_half']['mean']:.4f}" in stdout.splitlines()
    # without the flag: the existing keys only, with identical values
    plain, plain_out = runs["plain"]
    assert list(plain["metrics"]) == EXISTING_KEYS
    assert {k: m["metrics"][k] for k in EXISTING_KEYS} == plain["metrics"]
    assert "view retrieval" not in plain_out and "counterfactual" not in plain_out
    for key in ("kind", "version", "step", "scale_aware", "seed", "val_slices", "datasets", "model"):
        assert m[key] == plain[key]
    # --skip-view-retrieval: no key, the reference's SKIPPED line, metric 3 as before
    skip, skip_out = runs["skip"]
    assert list(skip["metrics"]) == EXISTING_KEYS + ["spacing_counterfactual"]
    assert any(ln.endswith("Per-dataset view retrieval... SKIPPED (--skip-view-retrieval)") for ln in skip_out.splitlines())
    assert skip["metrics"]["spacing_counterfactual"] == cf
