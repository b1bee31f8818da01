"""CPU checks of the nearest-neighbour evaluation: ``dinox.neighbors`` with ``ops.knn_topk`` replaced by a NumPy float64 top-k (the golden
fixture's recorded reference result, a hand-computed vote), the argument checking of ``ops.knn_topk``, the host-side validation of
the library entry, and the flag surface of scripts/evaluate_panorgan.py.  No kernel is launched."""
import importlib.util
import json
import os
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

SCRIPT = os.path.join(ROOT, "dino-x_amd", "scripts", "evaluate_panorgan.py")

# flag -> default of the reference's parser, for the flags that apply (--split-manifest is required there; here --synthetic replaces it)
REFERENCE_FLAGS = {
    "--checkpoint": None, "--index-csv": Path("data/processed/combined-mvp/index.csv"), "--split-manifest": None, "--scale-aware": False,
    "--out": None, "--batch-size": 64, "--seed": 42, "--device": None,
}


def host_knn_topk(q, k, K, exclude=None):
    """NumPy float64 stand-in for ops.knn_topk: (score descending, index ascending), exclude[i] left out, (-1, -inf) padding."""
    qn, kn = q.cpu().numpy().astype(np.float64), k.cpu().numpy().astype(np.float64)
    S = qn @ kn.T
    if isinstance(exclude, str):
        assert exclude == "self" and S.shape[0] == S.shape[1]
        np.fill_diagonal(S, -np.inf)
    elif exclude is not None:
        for i, j in enumerate(exclude.tolist()):
            if 0 <= j < S.shape[1]:
                S[i, j] = -np.inf
    order = np.argsort(-S, axis=1, kind="stable")[:, :K]
    val = np.take_along_axis(S, order, 1)
    idx = np.where(np.isneginf(val), -1, order)
    pad = K - idx.shape[1]
    if pad > 0:
        idx = np.concatenate([idx, np.full((idx.shape[0], pad), -1)], 1)
        val = np.concatenate([val, np.full((val.shape[0], pad), -np.inf)], 1)
    return torch.from_numpy(idx.astype(np.int32)), torch.from_numpy(val.astype(np.float32))


@pytest.fixture
def neighbors(monkeypatch):
    from dinox import neighbors, ops
    monkeypatch.setattr(ops, "knn_topk", host_knn_topk)
    return neighbors


@pytest.fixture(scope="module")
def script():
    spec = importlib.util.spec_from_file_location("evaluate_panorgan", SCRIPT)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_fixture():
    z = np.load(os.path.join(GOLDEN, "domain_clustering.npz"))
    names = [str(s) for s in z["label_names"]]
    return z, z["rows"], [names[i] for i in z["labels"]], json.loads(str(z["reference_result"]))


def same(got, want, path=""):
    """Counts and strings exactly, rates and ratios to 1e-12."""
    if isinstance(want, dict):
        assert list(got) == list(want), (path, list(got), list(want))
        for key in want:
            same(got[key], want[key], f"{path}/{key}")
    elif isinstance(want, float):
        assert isinstance(got, float) and abs(got - want) <= 1e-12, (path, got, want)
    else:
        assert type(got) is type(want) and got == want, (path, got, want)


# ------------------------------------------------------------------------------------------ fixture
def test_fixture_has_one_right_answer():
    """What the generator asserts, re-checked on the committed file: class-by-class storage, the cluster sizes, a rate clearly between
    random and 1, and -- for every row -- one label among all keys within tau of the 10th float64 score."""
    z, rows, labels, want = load_fixture()
    assert rows.shape == (1536, 64) and rows.dtype == np.float32 and np.allclose(np.linalg.norm(rows, axis=1), 1.0, atol=1e-6)
    lab = z["labels"]
    assert np.array_equal(lab, np.repeat(np.arange(4), (640, 512, 256, 128)))
    assert abs(want["expected_random_rate"] - sum((n / 1536.0) ** 2 for n in (640, 512, 256, 128))) <= 1e-12
    assert 0.75 <= want["overall_same_dataset_rate"] <= 0.92 and want["k"] == 10
    tau = 2.0 * 64 * 2.0 ** -24
    S = rows.astype(np.float64) @ rows.astype(np.float64).T
    np.fill_diagonal(S, -np.inf)
    s10 = -np.sort(-S, axis=1)[:, 9]
    near = np.abs(S - s10[:, None]) <= tau
    assert all(len(set(lab[near[i]])) == 1 for i in range(1536))


def test_domain_clustering_reproduces_recorded_reference_result(neighbors):
    _, rows, labels, want = load_fixture()
    got = neighbors.domain_clustering(torch.from_numpy(rows), labels, k=10)
    same(got, want)
    assert list(got) == ["k", "overall_same_dataset_rate", "expected_random_rate", "enrichment_vs_random", "per_dataset", "note"]
    # None -> "unknown", as the reference's `r.dataset or "unknown"`
    some = [None if name == "head_ct" else name for name in labels]
    got = neighbors.domain_clustering(torch.from_numpy(rows), some, k=10)
    assert got["per_dataset"]["unknown"] == want["per_dataset"]["head_ct"] and "head_ct" not in got["per_dataset"]
    with pytest.raises(ValueError, match="labels"):
        neighbors.domain_clustering(torch.from_numpy(rows), labels[:-1])
    with pytest.raises(ValueError, match="k = 8"):
        neighbors.domain_clustering(torch.from_numpy(rows[:8]), labels[:8], k=8)


def test_knn_probe_hand_computed_example(neighbors):
    """Six unit rows in the plane at angles 0, 20, 45, 95, 180, 200 degrees, classes a a b b c c, leave-one-out, k = 3 (no two angle
    differences of a row coincide among its first four neighbours, so the neighbour sets are safe in any precision).  By hand, with
    w(x) = exp(cos(x deg) / T) and T = 1 (w(20) = 2.559, w(25) = 2.475, w(45) = 2.028, w(50) = 1.902, w(75) = 1.296, w(85) = 1.091,
    w(95) = 0.917, w(105) = 0.772, w(135) = 0.493, w(155) = 0.404):
      row 0 (a):  20 a, 45 b, 95 b        a 2.559 < b 2.945      -> b   wrong   (two weaker votes beat the nearest neighbour)
      row 1 (a):  20 a, 25 b, 75 b        a 2.559 < b 3.771      -> b   wrong
      row 2 (b):  25 a, 45 a, 50 b        a 4.503 > b 1.902      -> a   wrong
      row 3 (b):  50 b, 75 a, 85 c        b 1.902 > a 1.296 > c  -> b   right
      row 4 (c):  20 c, 85 b, 135 b       c 2.559 > b 1.584      -> c   right
      row 5 (c):  20 c, 105 b, 155 b      c 2.559 > b 1.176      -> c   right
    At T = 0.07 the nearest neighbour dominates (w(20) / w(25) = e^0.48, w(45) and beyond are e^-3 and less of it): rows 0 and 1 turn to a.
    Then an exact vote tie: two neighbours at the same similarity with different classes -> the lower class id."""
    ang = np.deg2rad([0.0, 20.0, 45.0, 95.0, 180.0, 200.0])
    x = torch.from_numpy(np.stack([np.cos(ang), np.sin(ang)], 1).astype(np.float32))
    y = ["a", "a", "b", "b", "c", "c"]
    got = neighbors.knn_probe(x, y, k=3, temperature=1.0, return_predictions=True)
    assert got["predictions"] == ["b", "b", "a", "b", "c", "c"]
    assert got["accuracy"] == 0.5 and got["per_class_accuracy"] == {"a": 0.0, "b": 0.5, "c": 1.0}
    assert got["classes"] == ["a", "b", "c"] and got["k"] == 3 and got["temperature"] == 1.0 and got["n_train"] == 6 and got["n_test"] == 6
    assert list(got)[:7] == ["accuracy", "per_class_accuracy", "k", "temperature", "n_train", "n_test", "classes"]
    assert "predictions" not in neighbors.knn_probe(x, y, k=3, temperature=1.0)
    got = neighbors.knn_probe(x, y, k=3, temperature=0.07, return_predictions=True)
    assert got["predictions"] == ["a", "a", "a", "b", "c", "c"] and got["accuracy"] == 5.0 / 6.0
    # exact tie: the test row (1, 0) sees train rows (0, 1) of class "z" and (0, -1) of class "m" at the same similarity 0
    tr = torch.tensor([[0.0, 1.0], [0.0, -1.0]])
    got = neighbors.knn_probe(tr, ["z", "m"], torch.tensor([[1.0, 0.0]]), k=2, temperature=0.07, test_labels=["z"], return_predictions=True)
    assert got["classes"] == ["m", "z"] and got["predictions"] == ["m"] and got["accuracy"] == 0.0 and got["n_train"] == 2 and got["n_test"] == 1
    # fewer eligible train rows than k: the missing neighbours do not vote (5 neighbours each; the defaults are k = 20, T = 0.07)
    got = neighbors.knn_probe(x, y, return_predictions=True)
    assert got["k"] == 20 and got["temperature"] == 0.07 and got["predictions"] == ["a", "a", "a", "b", "c", "c"]
    with pytest.raises(ValueError, match="test_labels"):
        neighbors.knn_probe(x, y, x)
    with pytest.raises(ValueError, match="temperature"):
        neighbors.knn_probe(x, y, temperature=0.0)


# ------------------------------------------------------------------------------------------ ops.knn_topk argument checking
def test_knn_topk_argument_errors_without_a_device():
    from dinox import ops
    z = torch.zeros(4, 8)
    with pytest.raises(ValueError, match=r"fp32 \[Nq, D\] and \[Nk, D\].*\(4, 8\)"):
        ops.knn_topk(z.bfloat16(), z, 2)
    with pytest.raises(ValueError, match=r"fp32.*\(4, 8\).*\(4, 9\)"):
        ops.knn_topk(z, torch.zeros(4, 9), 2)                                  # different D
    with pytest.raises(ValueError, match="fp32"):
        ops.knn_topk(z[0], z, 2)                                               # not 2-D
    with pytest.raises(ValueError, match="empty operand"):
        ops.knn_topk(torch.zeros(0, 8), z, 2)
    with pytest.raises(ValueError, match="queries on cpu, keys on meta"):
        ops.knn_topk(z, torch.zeros(4, 8, device="meta"), 2)
    for K in (0, 33, -3, 2.0, True, None):
        with pytest.raises(ValueError, match=r"K must be an integer in \[1, 32\].*\(4, 8\)"):
            ops.knn_topk(z, z, K)
    with pytest.raises(ValueError, match=r"exclude='self'.*Nq == Nk \(4, 5\)"):
        ops.knn_topk(z, torch.zeros(5, 8), 2, exclude="self")
    with pytest.raises(ValueError, match="exclude must be None, 'self'"):
        ops.knn_topk(z, z, 2, exclude="diagonal")
    with pytest.raises(ValueError, match=r"exclude must have shape \(4,\), got \(3,\)"):
        ops.knn_topk(z, z, 2, exclude=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="int32 or int64"):
        ops.knn_topk(z, z, 2, exclude=torch.zeros(4))
    # a well-formed call on host tensors reaches the device check: there is no CPU path
    for exclude in (None, "self", torch.zeros(4, dtype=torch.int64)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.knn_topk(z, z, 2, exclude=exclude)
    for K in (np.int64(2), np.int32(32)):                                      # NumPy integers are integers
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.knn_topk(z, z, K)


def test_knn_entry_validates_arguments_on_the_host():
    """Argument validation happens before any launch: safe without a GPU."""
    from dinox import _lib
    L = _lib.lib
    assert L.dinox_knn_ws_bytes(0, 4, 8, 10) == 0 and L.dinox_knn_ws_bytes(4, 4, 8, 0) == 0 and L.dinox_knn_ws_bytes(4, 4, 8, 33) == 0
    assert L.dinox_knn_ws_bytes(1, 1, 1, 1) == 8
    for n in (4096, 16384, 65536):                                             # 8 K bytes per query and key split, never more splits than the rank kernel
        for K in (10, 32):
            b = L.dinox_knn_ws_bytes(n, n, 384, K)
            assert b % (8 * K * n) == 0 and 1 <= b // (8 * K * n) <= L.dinox_retrieval_ws_bytes(n, n, 384) // (12 * n), (n, K, b)
    assert L.dinox_knn_ws_bytes(2 ** 31 - 100, 4, 8, 10) == 0 and L.dinox_knn_ws_bytes(4, 2 ** 31 - 100, 8, 10) == 0     # sizes the call refuses
    for K in (0, 33, -1):
        rc = L.dinox_knn_topk(16, 8, 16, 8, None, 4, 4, 8, K, 16, 16, 16, None)
        assert rc == -1 and f"K={K}" in _lib.last_error()
    rc = L.dinox_knn_topk(None, 8, None, 8, None, 4, 4, 8, 10, None, None, None, None)
    assert rc == -1 and "null pointer" in _lib.last_error()
    rc = L.dinox_knn_topk(16, 4, 16, 8, None, 4, 5, 8, 10, 16, 16, 16, None)
    assert rc == -1 and "ldq" in _lib.last_error()


# ------------------------------------------------------------------------------------------ deterministic evaluation view
def test_eval_view_is_the_fixed_window_centred_square_unflipped():
    from dinox.retrieval import eval_view
    for H, W in [(35, 35), (512, 512), (300, 200), (200, 300), (301, 200), (200, 301), (7, 4), (1, 9)]:
        v = eval_view(H, W)
        side = min(H, W)
        assert (v.level, v.width, v.flip) == (40.0, 400.0, False)
        assert (v.h, v.w) == (side, side) and 0 <= v.top and v.top + side <= H and 0 <= v.left and v.left + side <= W
        assert v.top == (H - side) // 2 and v.left == (W - side) // 2          # centred: the margins differ by at most one pixel
        assert abs((H - side - v.top) - v.top) <= 1 and abs((W - side - v.left) - v.left) <= 1
        assert v.top == 0 or v.left == 0                                       # the shorter side is kept whole


# ------------------------------------------------------------------------------------------ script
def test_script_flag_surface(script):
    ap = script.build_parser()
    have = {s for a in ap._actions for s in a.option_strings if s.startswith("--")} - {"--help"}
    assert set(REFERENCE_FLAGS) <= have
    assert have - set(REFERENCE_FLAGS) == {"--synthetic", "--amp-dtype", "--dump-embeddings"}        # the documented extensions
    d = vars(ap.parse_args(["--checkpoint", "x.pth"]))
    for flag, default in REFERENCE_FLAGS.items():
        if flag != "--checkpoint":
            assert d[flag[2:].replace("-", "_")] == default, flag
    assert d["checkpoint"] == Path("x.pth") and d["synthetic"] == 0 and d["amp_dtype"] == "fp32" and d["dump_embeddings"] is None
    with pytest.raises(SystemExit):
        ap.parse_args([])                                                      # --checkpoint is required
    with pytest.raises(SystemExit):
        ap.parse_args(["--checkpoint", "x.pth", "--amp-dtype", "fp16"])


def test_script_synthetic_labels(script):
    labels = [script.synthetic_label(i) for i in range(256)]
    names, counts = np.unique(labels, return_counts=True)
    assert len(names) >= 3 and len(set(counts.tolist())) == len(counts)       # at least three classes of unequal size
    assert labels == [script.synthetic_label(i) for i in range(256)]           # a function of i alone


def test_script_has_no_cpu_compute_path(script, tmp_path):
    ckpt = tmp_path / "checkpoint_00000001.pth"
    ckpt.write_bytes(b"")                                                      # never read: the device check comes first
    with pytest.raises(SystemExit, match="computes on MI355X only"):
        script.main(["--checkpoint", str(ckpt), "--synthetic", "64", "--device", "cpu"])
    with pytest.raises(FileNotFoundError):
        script.main(["--checkpoint", str(tmp_path / "missing.pth"), "--synthetic", "64"])
    with pytest.raises(SystemExit, match="split-manifest"):
        script.main(["--checkpoint", str(ckpt)])
