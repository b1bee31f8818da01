"""GPU tests of the top-K nearest-neighbour kernel (csrc/knn.hip, ``ops.knn_topk``) and the evaluation built on it (dinox/neighbors.py,
scripts/evaluate_panorgan.py).  Run with ``-m gpu`` on an MI355X.

1. exact case: integer-valued fp32 rows in {-3..3} make every score an exact integer (ties everywhere): indices and values must EQUAL a
   host ``np.lexsort((index, -score))`` top-K -- no tolerance;
2. float case: clustered unit rows against float64 scores, with the set interval the fp32 chain error allows, and a sharpness condition;
3. consistency with ``retrieval_rank`` (bitwise column 0), duplicated keys, run-to-run identity, strided views;
4. order independence under a permutation of the keys;
5. the metrics on the golden fixture against the recorded reference result and a float64 host vote;
6. the script on a reference-written checkpoint, its number checked against a float64 ranking of its own embeddings.
"""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

DEV = "cuda"
KS = (1, 10, 20, 32)


@pytest.fixture(scope="module")
def ops():
    from dinox import ops
    import dinox._lib as L
    assert L.lib.dinox_device_ok() == 1, L.last_error()
    return ops


def run_knn(ops, q, k, K, exclude=None):
    tq, tk = torch.from_numpy(q).to(DEV), torch.from_numpy(k).to(DEV)
    ex = torch.from_numpy(exclude).to(DEV) if isinstance(exclude, np.ndarray) else exclude
    idx, val = ops.knn_topk(tq, tk, K, exclude=ex)
    torch.cuda.synchronize()
    assert idx.dtype == torch.int32 and val.dtype == torch.float32 and idx.shape == (q.shape[0], K) and val.shape == (q.shape[0], K)
    return idx.cpu().numpy(), val.cpu().numpy()


def host_topk(S, order, K, exclude):
    """First K entries per row of ``order`` (= every row's keys sorted by (score descending, index ascending)) after dropping key
    exclude[i]; slots past the eligible keys hold (-1, -inf).  Values in S's dtype."""
    Nq, Nk = S.shape
    idx = np.full((Nq, K), -1, dtype=np.int64)
    val = np.full((Nq, K), -np.inf, dtype=np.float64)
    take = order[:, :K + 1]                                   # at most one key of a row is excluded
    keep = take != (np.full(Nq, -1) if exclude is None else exclude.astype(np.int64))[:, None]
    place = np.cumsum(keep, axis=1) - 1
    r, c = np.nonzero(keep & (place < K))
    idx[r, place[r, c]] = take[r, c]
    val[r, place[r, c]] = S[r, take[r, c]]
    return idx, val


def full_order(S):
    """A stable argsort of -S is np.lexsort((index, -score)) row by row (checked on a few rows)."""
    order = np.argsort(-S, axis=1, kind="stable")
    index = np.arange(S.shape[1])
    for i in sorted({0, S.shape[0] // 2, S.shape[0] - 1}):
        assert np.array_equal(order[i], np.lexsort((index, -S[i])))
    return order


# ------------------------------------------------------------------------------------------ 1. exact
EXACT_SHAPES = [(4096, 4096, 384), (777, 1029, 384), (129, 4099, 1024), (1000, 1000, 88), (1, 1, 1), (300, 65, 7), (5, 3, 16)]


def integer_rows(Nq, Nk, D):
    g = np.random.default_rng(Nq * 7 + Nk * 3 + D)
    q = g.integers(-3, 4, (Nq, D)).astype(np.float32)
    k = g.integers(-3, 4, (Nk, D)).astype(np.float32)
    # |s| <= 9 D < 2^14 and every partial sum is an integer: the float64 BLAS product is the exact integer result
    S = (q.astype(np.float64) @ k.astype(np.float64).T).astype(np.int64)
    return g, q, k, S


@pytest.mark.parametrize("Nq,Nk,D", EXACT_SHAPES)
def test_exact_integer_topk(ops, Nq, Nk, D):
    g, q, k, S = integer_rows(Nq, Nk, D)
    order = full_order(S)
    rnd = g.integers(-1, Nk, Nq).astype(np.int32)             # includes -1 (nothing) ...
    rnd[::7] = Nk + g.integers(0, 5, len(rnd[::7]))            # ... and out-of-range values, which exclude nothing
    rnd[::11] = -5 - g.integers(0, 5, len(rnd[::11]))
    rnd64 = rnd.astype(np.int64)
    rnd64[::7] = 2 ** 32 + g.integers(0, Nk, len(rnd64[::7]))  # (int64 indices that would wrap into range as int32)
    cases = [("None", None, None), ("random", rnd, np.where((rnd >= 0) & (rnd < Nk), rnd, -1)),
             ("random64", rnd64, np.where((rnd64 >= 0) & (rnd64 < Nk), rnd64, -1))]
    if Nq == Nk:
        cases.append(("self", "self", np.arange(Nq)))
    for K in KS:
        for name, exclude, eff in cases:
            idx, val = run_knn(ops, q, k, K, exclude)
            want_idx, want_val = host_topk(S, order, K, eff)
            what = f"({Nq}, {Nk}, {D}) K={K} exclude={name}"
            print(f"{what}: index mismatches {int((idx != want_idx).sum())}, value mismatches {int((val != want_val).sum())}")
            assert np.array_equal(idx.astype(np.int64), want_idx), what
            assert np.array_equal(val.astype(np.float64), want_val), what                 # -inf == -inf in the padding
            if Nk < K:
                assert (idx[:, -1] == -1).all() and np.isneginf(val[:, -1]).all(), what


def test_k_range_and_bad_shapes_are_refused(ops):
    z = torch.zeros(4, 8, device=DEV)
    for K in (0, 33, -1):
        with pytest.raises(ValueError, match="K must be"):
            ops.knn_topk(z, z, K)
    with pytest.raises(ValueError, match="needs Nq == Nk"):
        ops.knn_topk(z, torch.zeros(5, 8, device=DEV), 2, exclude="self")
    with pytest.raises(ValueError, match="exclude must have shape"):
        ops.knn_topk(z, z, 2, exclude=torch.zeros(3, dtype=torch.int32, device=DEV))
    from dinox import _lib
    L = _lib.lib
    for K in (0, 33):                                         # the library refuses by return code, before any launch
        assert L.dinox_knn_topk(z.data_ptr(), 8, z.data_ptr(), 8, None, 4, 4, 8, K, z.data_ptr(), z.data_ptr(), z.data_ptr(), None) == -1
        assert "K=" in _lib.last_error()
    # every score ties: plain index order, self left out
    idx, val = ops.knn_topk(z, z, 3, exclude="self")
    assert idx.tolist() == [[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]] and not val.any()


def test_nan_rows_neither_fault_nor_hang(ops):
    g = torch.Generator().manual_seed(1)
    q, k = torch.randn(70, 16, generator=g), torch.randn(300, 16, generator=g)
    q[2] = float("nan")
    k[17, 3] = float("nan")
    idx, val = ops.knn_topk(q.to(DEV), k.to(DEV), 10)
    torch.cuda.synchronize()
    idx, val = idx.cpu().numpy(), val.cpu().numpy()
    assert (idx >= -1).all() and (idx < 300).all()
    assert (idx[2] == -1).all() and np.isneginf(val[2]).all()                               # documented in dinox.h
    ok = np.arange(70) != 2
    assert not (idx[ok] == 17).any() and (idx[ok] >= 0).all() and np.isfinite(val[ok]).all()


# ------------------------------------------------------------------------------------------ 2. float
def clustered_rows(N, D):
    """The q rows of tests/test_retrieval_gpu.py::clustered_views(N, D, .), restated: x = c[label] + 0.7 n1, unit(x); 64 clusters;
    fixed seed and draw order.  Also returns the cluster of every row."""
    g = np.random.default_rng(7)
    c = g.standard_normal((64, D))
    label = g.integers(0, 64, N)
    n1 = g.standard_normal((N, D))
    g.standard_normal((N, D))                                 # (n2 of the original: drawn there, not used for q)
    x = c[label] + 0.7 * n1
    return (x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-12)).astype(np.float32), label


def check_float_rows(x, idx, val, K, D, what):
    """The conditions of the float case for keys = queries = x, self excluded.  Returns the share of rows with one admissible set."""
    N = x.shape[0]
    eps = D * 2.0 ** -24
    tau = 2.0 * eps
    S = x.astype(np.float64) @ x.astype(np.float64).T
    np.fill_diagonal(S, -np.inf)
    top = -np.sort(-S, axis=1)[:, :K + 1]
    sK, sK1 = top[:, K - 1], top[:, K]
    sharp = float(((sK - sK1) > 2 * tau).mean())
    rows = np.arange(N)[:, None]
    assert (idx >= 0).all() and (idx < N).all() and (idx != rows).all(), what
    assert all(len(set(r)) == K for r in idx), what                                        # no key twice
    got = S[rows, idx]
    low = int((got < sK[:, None] - tau).sum())
    hit = np.zeros((N, N), dtype=bool)
    hit[rows, idx] = True
    missed = int(((S > sK[:, None] + tau) & ~hit).sum())
    err = float(np.abs(val - got).max())
    dv = np.diff(val.astype(np.float64), axis=1)
    disorder = int((dv > 0).sum() + ((dv == 0) & (np.diff(idx, axis=1) <= 0)).sum())
    print(f"{what}: rows with one admissible set {100 * sharp:.2f} %, keys below s_K - tau {low}, keys above s_K + tau missed {missed}, "
          f"max |val - S64| {err:.3e} (eps {eps:.3e}), order violations {disorder}")
    assert low == 0 and missed == 0 and err <= eps and disorder == 0, what
    return sharp


@pytest.mark.parametrize("K", [10, 20, 32])
@pytest.mark.parametrize("layout", ["shuffled", "by_cluster"])
def test_float_topk_within_derived_interval(ops, K, layout):
    x, label = clustered_rows(4096, 384)
    if layout == "by_cluster":                                # the unfriendly order: a query's own cluster may come last
        x = np.ascontiguousarray(x[np.argsort(label, kind="stable")])
    idx, val = run_knn(ops, x, x, K, "self")
    sharp = check_float_rows(x, idx, val, K, 384, f"clustered rows {layout} K={K}")
    assert sharp >= 0.85, sharp                               # a property of the input: 0.93 / 0.90 / 0.89 at K = 10 / 20 / 32


# ------------------------------------------------------------------------------------------ 3. consistency
def bits(a):
    return a.view(np.uint32)


def test_column_zero_is_retrieval_rank_best(ops):
    x, _ = clustered_rows(2053, 1024)
    g = np.random.default_rng(3)
    y = x[g.permutation(2053)] + 0.05 * g.standard_normal((2053, 1024)).astype(np.float32)
    for q, k in ((x, y), (x, x)):
        tq, tk = torch.from_numpy(q).to(DEV), torch.from_numpy(k).to(DEV)
        _, best_idx, best_val, _ = ops.retrieval_rank(tq, tk)
        for K in (1, 10, 32):
            idx, val = ops.knn_topk(tq, tk, K)
            assert torch.equal(idx[:, 0], best_idx)
            assert np.array_equal(bits(val[:, 0].cpu().numpy()), bits(best_val.cpu().numpy()))
    _, q, k, _ = integer_rows(515, 901, 96)                   # the exact case too, where many keys share the maximum
    tq, tk = torch.from_numpy(q).to(DEV), torch.from_numpy(k).to(DEV)
    _, bi, bv, _ = ops.retrieval_rank(tq, tk, torch.zeros(515, dtype=torch.int32, device=DEV))
    idx, val = ops.knn_topk(tq, tk, 20)
    assert torch.equal(idx[:, 0], bi) and torch.equal(val[:, 0], bv)


def test_duplicated_keys_are_adjacent_lower_index_first(ops):
    x, _ = clustered_rows(1000, 88)
    k = x.copy()
    k[500:] = k[:500]                                         # key 500 + i is bitwise key i
    for K in (10, 32):
        idx, val = run_knn(ops, x, k, K)
        pairs = 0
        for i in range(1000):
            for p in range(K - 1):
                if idx[i, p] < 500:                           # its twin follows at once, with the same bits
                    assert idx[i, p + 1] == idx[i, p] + 500 and bits(val[i])[p + 1] == bits(val[i])[p], (i, p, idx[i], val[i])
                    pairs += 1
            hi = idx[i][idx[i] >= 500]
            assert np.isin(hi - 500, idx[i]).all() and (idx[i, 0] < 500)       # a twin never comes without / before its original
        assert pairs >= 1000 * (K // 2 - 1)


def test_two_runs_are_bit_identical_and_strided_views_equal_copies(ops):
    x, _ = clustered_rows(4096, 384)
    a, b = run_knn(ops, x, x, 20, "self"), run_knn(ops, x, x, 20, "self")
    assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))
    g = np.random.default_rng(11)
    for Nq, Nk, D, pad, off in [(200, 333, 64, 16, 0), (200, 333, 64, 3, 1), (130, 130, 40, 8, 4)]:
        qb = g.standard_normal((Nq, D + pad)).astype(np.float32)
        kb = g.standard_normal((Nk, D + pad)).astype(np.float32)
        tq, tk = torch.from_numpy(qb).to(DEV)[:, off:off + D], torch.from_numpy(kb).to(DEV)[:, off:off + D]
        assert not tq.is_contiguous()
        i1, v1 = ops.knn_topk(tq, tk, 10)
        i2, v2 = ops.knn_topk(tq.contiguous(), tk.contiguous(), 10)
        assert torch.equal(i1, i2) and np.array_equal(bits(v1.cpu().numpy()), bits(v2.cpu().numpy()))


# ------------------------------------------------------------------------------------------ 4. order independence
def sets_by_score(idx, val):
    """Per row: {score: set of keys} for the scores strictly above the row's last one (the last score's set may be cut by K)."""
    out = []
    for r_i, r_v in zip(idx, val):
        d = {}
        for j, v in zip(r_i, r_v):
            if v > r_v[-1]:
                d.setdefault(float(v), set()).add(int(j))
        out.append(d)
    return out


@pytest.mark.parametrize("data", ["integer", "clustered_by_cluster"])
def test_key_order_does_not_matter(ops, data):
    if data == "integer":
        _, q, k, _ = integer_rows(777, 1029, 384)
    else:
        x, label = clustered_rows(4096, 384)
        q = k = np.ascontiguousarray(x[np.argsort(label, kind="stable")])
    Nk = k.shape[0]
    for seed, K in ((0, 10), (1, 32)):
        perm = np.random.default_rng(seed).permutation(Nk)
        if seed == 1:
            perm = perm[::-1].copy() if data == "integer" else np.arange(Nk)[::-1].copy()    # all good candidates late / at once
        idx0, val0 = run_knn(ops, q, k, K)
        idxp, valp = run_knn(ops, q, np.ascontiguousarray(k[perm]), K)
        back = perm[idxp]                                     # key j of the permuted call is key perm[j]
        assert np.array_equal(bits(val0), bits(valp)), data   # same keys, same chain per score: the ordered values agree bitwise
        a, b = sets_by_score(idx0, val0), sets_by_score(back, valp)
        assert a == b, data
        # and each call is the exact order of its own key numbering
        for idx, val in ((idx0, val0), (idxp, valp)):
            dv = np.diff(val.astype(np.float64), axis=1)
            assert not (dv > 0).any() and not ((dv == 0) & (np.diff(idx, axis=1) <= 0)).any()


# ------------------------------------------------------------------------------------------ 5. metrics end to end
def load_fixture():
    z = np.load(os.path.join(GOLDEN, "domain_clustering.npz"))
    names = [str(s) for s in z["label_names"]]
    return z["rows"], [names[i] for i in z["labels"]], json.loads(str(z["reference_result"]))


def same(got, want, path=""):
    """Counts and strings exactly, rates and ratios to 1e-12."""
    assert type(got) is type(want) or {type(got), type(want)} <= {int, float}, (path, got, want)
    if isinstance(want, dict):
        assert list(got) == list(want), (path, list(got), list(want))
        for key in want:
            same(got[key], want[key], f"{path}/{key}")
    elif isinstance(want, float):
        assert abs(got - want) <= 1e-12, (path, got, want)
    else:
        assert got == want, (path, got, want)


def test_domain_clustering_on_fixture_equals_recorded_reference(ops):
    from dinox import neighbors
    rows, labels, want = load_fixture()
    got = neighbors.domain_clustering(torch.from_numpy(rows).to(DEV), labels, k=10)
    print(f"domain_clustering on the fixture: overall {got['overall_same_dataset_rate']:.6f} (reference {want['overall_same_dataset_rate']:.6f})")
    same(got, want)


def host_vote(S, train_id, n_classes, k, T):
    """The weighted vote in float64 on exact float64 scores (self already masked in S): (prediction, winning margin relative to the
    total vote) per row."""
    order = np.argsort(-S, axis=1, kind="stable")[:, :k]
    s = np.take_along_axis(S, order, 1)
    w = np.exp(s / T)
    votes = np.zeros((S.shape[0], n_classes))
    for p in range(k):
        votes[np.arange(S.shape[0]), train_id[order[:, p]]] += w[:, p]
    srt = np.sort(votes, axis=1)
    return np.argmax(votes, axis=1), (srt[:, -1] - srt[:, -2]) / votes.sum(1), s


def test_knn_probe_on_fixture_matches_float64_vote(ops):
    """Bound on what eps = D 2^-24 in the k scores can move: a score off by at most eps changes its weight exp(s / T) by a factor within
    exp(+-eps / T), and a neighbour swapped for another inside tau = 2 eps of the k-th score changes at most ONE vote of weight
    <= exp((s_k + tau) / T) per swap.  Rows are compared when (a) the k-th and (k+1)-th float64 scores are more than 2 tau apart (the
    neighbour set is unique: no swap) and (b) the relative winning margin exceeds 2 (exp(eps / T) - 1) (every vote sum moves by at most
    that fraction of the total).  The rest is counted: at most 1 % of the rows."""
    from dinox import neighbors
    rows, labels, _ = load_fixture()
    k, T, D = 20, 0.07, rows.shape[1]
    eps = D * 2.0 ** -24
    tau = 2 * eps
    got = neighbors.knn_probe(torch.from_numpy(rows).to(DEV), labels, k=k, temperature=T, return_predictions=True)
    classes = sorted(set(labels))
    assert got["classes"] == classes and got["k"] == k and got["temperature"] == T and got["n_train"] == got["n_test"] == len(labels)
    train_id = np.array([classes.index(c) for c in labels])
    S = rows.astype(np.float64) @ rows.astype(np.float64).T
    np.fill_diagonal(S, -np.inf)
    s = -np.sort(-S, axis=1)[:, :k + 1]                       # the k + 1 best float64 scores per row
    pred, margin, _ = host_vote(S, train_id, len(classes), k, T)
    decided = ((s[:, k - 1] - s[:, k]) > 2 * tau) & (margin > 2 * np.expm1(eps / T))
    left_out = int((~decided).sum())
    got_id = np.array([classes.index(c) for c in got["predictions"]])
    wrong = int((got_id[decided] != pred[decided]).sum())
    print(f"knn_probe on the fixture: accuracy {got['accuracy']:.6f}, float64 vote {float((pred == train_id).mean()):.6f}, rows left out "
          f"{left_out} of {len(labels)}, disagreements among the rest {wrong}")
    assert left_out <= 0.01 * len(labels)
    assert wrong == 0
    if left_out == 0:
        assert got["accuracy"] == float(np.mean(pred == train_id))
        for ci, c in enumerate(classes):
            assert got["per_class_accuracy"][c] == float(np.mean(pred[train_id == ci] == ci))
    # a held-out split goes through the same vote: the fixture's even rows classify its odd rows
    tr, te = np.arange(0, len(labels), 2), np.arange(1, len(labels), 2)
    got2 = neighbors.knn_probe(torch.from_numpy(rows[tr]).to(DEV), [labels[i] for i in tr], torch.from_numpy(rows[te]).to(DEV), k=k,
                               temperature=T, test_labels=[labels[i] for i in te], return_predictions=True)
    S2 = rows[te].astype(np.float64) @ rows[tr].astype(np.float64).T
    s2 = -np.sort(-S2, axis=1)[:, :k + 1]
    pred2, margin2, _ = host_vote(S2, train_id[tr], len(classes), k, T)
    decided2 = ((s2[:, k - 1] - s2[:, k]) > 2 * tau) & (margin2 > 2 * np.expm1(eps / T))
    got2_id = np.array([classes.index(c) for c in got2["predictions"]])
    assert (~decided2).sum() <= 0.01 * len(te) and np.array_equal(got2_id[decided2], pred2[decided2])
    assert got2["n_train"] == len(tr) and got2["n_test"] == len(te)


# ------------------------------------------------------------------------------------------ 6. script
ENVELOPE = ["kind", "version", "created_at", "checkpoint", "step", "scale_aware", "seed", "val_slices", "datasets", "model", "metrics",
            "seconds"]


def float64_topk(E, k):
    S = E.astype(np.float64) @ E.astype(np.float64).T
    np.fill_diagonal(S, -np.inf)
    return np.argsort(-S, axis=1, kind="stable")[:, :k], S


def test_script_on_reference_checkpoint(tmp_path, monkeypatch):
    from dinox import neighbors
    import dinox.ops
    ckpt = tmp_path / "ref_checkpoint_00000003.pth"
    shutil.copy(os.path.join(GOLDEN, "ref_checkpoint_00000003.pth"), ckpt)
    script = os.path.join(ROOT, "dino-x_amd", "scripts", "evaluate_panorgan.py")
    dump = tmp_path / "emb.npz"
    p = subprocess.run([sys.executable, script, "--checkpoint", str(ckpt), "--synthetic", "256", "--scale-aware", "--dump-embeddings", str(dump)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    print(p.stdout)
    print(p.stderr[-2000:])
    assert p.returncode == 0, p.stderr[-2000:]
    out = tmp_path / "panorgan_eval_step3.json"
    assert out.exists()
    m = json.loads(out.read_text())
    assert list(m) == ENVELOPE and m["kind"] == "panorgan_evaluation" and m["version"] == 1 and m["step"] == 3
    assert m["scale_aware"] is True and m["seed"] == 42 and m["val_slices"] == 256
    assert set(m["model"]) == {"name", "patch", "dim", "depth", "heads"} and m["model"]["dim"] == 32
    assert set(m["metrics"]) == {"domain_clustering", "knn_probe"}
    dc = m["metrics"]["domain_clustering"]
    assert list(dc) == ["k", "overall_same_dataset_rate", "expected_random_rate", "enrichment_vs_random", "per_dataset", "note"]
    assert dc["k"] == 10 and 0.0 <= dc["overall_same_dataset_rate"] <= 1.0
    z = np.load(dump)
    E, labels = z["embeddings"], [str(s) for s in z["labels"]]
    assert E.shape == (256, 32) and E.dtype == np.float32 and np.allclose(np.linalg.norm(E, axis=1), 1.0, atol=1e-6)
    names, counts = np.unique(labels, return_counts=True)
    assert len(names) >= 3 and len(set(counts.tolist())) == len(counts) and m["datasets"] == sorted(names.tolist())
    assert abs(dc["expected_random_rate"] - float(((counts / 256.0) ** 2).sum())) <= 1e-12
    for name, n in zip(names, counts):
        d = dc["per_dataset"][name]
        assert d["n"] == n and 0.0 <= d["same_dataset_rate"] <= 1.0 and abs(d["expected_random"] - n / 256.0) <= 1e-12
    lines = p.stdout.splitlines()
    assert f"  Same-dataset NN rate: {dc['overall_same_dataset_rate']:.3f}" in lines
    assert f"  Expected random: {dc['expected_random_rate']:.3f}" in lines and f"  Enrichment: {dc['enrichment_vs_random']:.1f}×" in lines
    assert lines[-1] == "ok=true"
    # the script's number against an independent float64 ranking of its own embeddings
    top, S = float64_topk(E, 11)
    tau = 2.0 * E.shape[1] * 2.0 ** -24
    lab = np.unique(labels, return_inverse=True)[1]
    s10 = S[np.arange(256), top[:, 9]]
    near = np.abs(S - s10[:, None]) <= tau                    # keys inside tau of the 10th score ...
    shaky = np.array([len(set(lab[near[i]])) > 1 for i in range(256)])       # ... that do not all carry one label
    print(f"rows inside tau of a label-changing tie: {int(shaky.sum())}")
    monkeypatch.setattr(dinox.ops, "knn_topk", lambda q, k, K, exclude=None: (torch.from_numpy(top[:, :K].astype(np.int32)), None))
    want = neighbors.domain_clustering(torch.from_numpy(E), labels, k=10)
    # a shaky row may move its own same-dataset share by at most 1, so a mean over n rows by at most (shaky rows among them) / n; with no
    # shaky row in a group the comparison is the exact one
    assert list(dc["per_dataset"]) == list(want["per_dataset"])
    for ci, name in enumerate(np.unique(labels)):
        got_d, want_d, members = dc["per_dataset"][name], want["per_dataset"][name], lab == ci
        slack = float(shaky[members].sum()) / float(members.sum())
        print(f"  {name}: n {int(members.sum())}, shaky rows {int(shaky[members].sum())}, rate {got_d['same_dataset_rate']:.6f} vs float64 "
              f"ranking {want_d['same_dataset_rate']:.6f}")
        assert got_d["n"] == want_d["n"] and abs(got_d["expected_random"] - want_d["expected_random"]) <= 1e-12
        assert abs(got_d["same_dataset_rate"] - want_d["same_dataset_rate"]) <= slack + 1e-12, name
    assert abs(dc["overall_same_dataset_rate"] - want["overall_same_dataset_rate"]) <= shaky.sum() / 256.0 + 1e-12
    assert dc["expected_random_rate"] == want["expected_random_rate"] and dc["k"] == want["k"] and dc["note"] == want["note"]
    if not shaky.any():
        same(dc, want)
    assert shaky.mean() <= 0.25                               # sharpness: the comparison is exact on at least three rows in four
    kp = m["metrics"]["knn_probe"]
    assert list(kp) == ["accuracy", "per_class_accuracy", "k", "temperature", "n_train", "n_test", "classes"]
    assert kp["k"] == 20 and kp["temperature"] == 0.07 and kp["n_train"] == kp["n_test"] == 256 and kp["classes"] == sorted(names.tolist())
    assert 0.0 <= kp["accuracy"] <= 1.0
