"""CPU checks of the view-retrieval evaluation: the metric block against a restatement of the reference's argmax / argpartition
block (scripts/phase5_view_retrieval_eval.py:214-236), and the flag surface of the drop-in script.  No kernel is launched."""
import importlib.util
import os
import sys
from pathlib import Path

import numpy as np
import pytest

from conftest import ROOT

SCRIPT = os.path.join(ROOT, "dino-x_amd", "scripts", "phase5_view_retrieval_eval.py")

# flag -> default of the reference's parser (required flags and --split-manifest have none: None)
REFERENCE_FLAGS = {
    "--checkpoint": None, "--index-csv": Path("data/processed/_index/index.csv"), "--split-manifest": None, "--n": 4096, "--seed": 0,
    "--batch-size": 64, "--device": None, "--out": None, "--topk": 5, "--ratio": 10.0, "--scale-aware": False,
}


@pytest.fixture(scope="module")
def script():
    spec = importlib.util.spec_from_file_location("phase5_view_retrieval_eval", SCRIPT)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def reference_metrics(S: np.ndarray, topk: int, ratio: float) -> dict:
    n = S.shape[0]
    top1 = float(np.mean(np.argmax(S, axis=1) == np.arange(n)))
    k = min(int(topk), n)
    topk_idx = np.argpartition(-S, kth=k - 1, axis=1)[:, :k]
    acc = float(np.mean([(i in topk_idx[i]) for i in range(n)]))
    baseline = 1.0 / float(n)
    return {"top1": top1, "topk_acc": acc, "random_baseline": baseline, "ratio_vs_random": top1 / baseline,
            "passed": bool(top1 >= float(ratio) * baseline)}


def stable_ranks(S: np.ndarray, target: np.ndarray) -> np.ndarray:
    """rank[i] = #{j : S[i,j] > S[i,t_i]} + #{j < t_i : S[i,j] == S[i,t_i]}."""
    pos = S[np.arange(S.shape[0]), target][:, None]
    before = np.arange(S.shape[1])[None, :] < target[:, None]
    return ((S > pos) | ((S == pos) & before)).sum(1)


@pytest.mark.parametrize("n,topk,ratio", [(1, 1, 10.0), (2, 5, 1.0), (7, 3, 2.0), (64, 5, 10.0), (64, 64, 10.0), (257, 5, 10.0),
                                          (257, 1000, 50.0), (1000, 1, 10.0), (1000, 17, 300.0)])
def test_metrics_from_ranks_matches_reference_block(n, topk, ratio):
    from dinox.retrieval import metrics_from_ranks
    g = np.random.default_rng(n * 1009 + topk)
    # float64 scores: tie-free (checked), the diagonal lifted so that top-1 is neither 0 nor 1
    S = g.standard_normal((n, n))
    S[np.arange(n), np.arange(n)] += g.uniform(0.0, 3.0, n)
    assert all(len(np.unique(row)) == n for row in S)
    rank = stable_ranks(S, np.arange(n))
    got = metrics_from_ranks(rank, topk, ratio)
    want = reference_metrics(S, topk, ratio)
    assert set(got) == set(want)
    for k in want:
        assert got[k] == want[k], (k, got[k], want[k])
    assert isinstance(got["passed"], bool) and isinstance(got["top1"], float)
    if n >= 64:
        assert 0.0 < got["top1"] < 1.0
    # any integer array type is taken (the kernel returns int32)
    assert metrics_from_ranks(rank.astype(np.int32), topk, ratio) == got


def test_metrics_from_ranks_rejects_empty_and_bad_topk():
    from dinox.retrieval import metrics_from_ranks
    with pytest.raises(ValueError):
        metrics_from_ranks(np.zeros(0, dtype=np.int32), 5, 10.0)
    with pytest.raises(ValueError):
        metrics_from_ranks(np.zeros(4, dtype=np.int32), 0, 10.0)


def test_script_flag_surface_matches_reference(script):
    ap = script.build_parser()
    have = {s for a in ap._actions for s in a.option_strings if s.startswith("--")} - {"--help"}
    assert set(REFERENCE_FLAGS) <= have
    assert have - set(REFERENCE_FLAGS) == {"--synthetic", "--amp"}                      # the documented extensions
    d = vars(ap.parse_args(["--checkpoint", "x.pth"]))
    for flag, default in REFERENCE_FLAGS.items():
        if flag != "--checkpoint":
            assert d[flag[2:].replace("-", "_")] == default, flag
    assert d["checkpoint"] == Path("x.pth") and d["synthetic"] == 0 and d["amp"] is False
    with pytest.raises(SystemExit):
        ap.parse_args([])                                                               # --checkpoint is required


def test_script_has_no_cpu_compute_path(script, tmp_path):
    ckpt = tmp_path / "checkpoint_00000001.pth"
    ckpt.write_bytes(b"")                                                               # never read: the device check comes first
    with pytest.raises(SystemExit, match="computes on MI355X only"):
        script.main(["--checkpoint", str(ckpt), "--synthetic", "8", "--device", "cpu"])
    with pytest.raises(FileNotFoundError):
        script.main(["--checkpoint", str(tmp_path / "missing.pth"), "--synthetic", "8"])
    with pytest.raises(SystemExit, match="split-manifest"):
        script.main(["--checkpoint", str(ckpt)])


def test_retrieval_rank_rejects_cpu_tensors():
    import torch
    from dinox import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.retrieval_rank(torch.zeros(4, 8), torch.zeros(4, 8))


def test_retrieval_entry_validates_arguments_on_the_host():
    """Argument validation happens before any launch: safe without a GPU."""
    from dinox import _lib
    L = _lib.lib
    assert L.dinox_retrieval_ws_bytes(0, 4, 8) == 0
    # 12 bytes per query and key split: O(Nq x splits), never O(Nq x Nk)
    assert L.dinox_retrieval_ws_bytes(1, 1, 1) == 12
    for n in (4096, 16384, 65536):
        b = L.dinox_retrieval_ws_bytes(n, n, 384)
        assert b % (12 * n) == 0 and 1 <= b // (12 * n) <= 64, (n, b)
    rc = L.dinox_retrieval_rank(None, 8, None, 8, None, 4, 4, 8, None, None, None, None, None, None)
    assert rc == -1 and "null pointer" in _lib.last_error()
    rc = L.dinox_retrieval_rank(16, 8, 16, 8, None, 4, 5, 8, 16, 16, 16, 16, 16, None)
    assert rc == -1 and "Nq == Nk" in _lib.last_error()
    rc = L.dinox_retrieval_rank(16, 4, 16, 8, 16, 4, 5, 8, 16, 16, 16, 16, 16, None)
    assert rc == -1 and "ldq" in _lib.last_error()


def test_exact_case_generator_has_ties():
    """tests/test_retrieval_gpu.py's exact case exercises the tie rule only if ties with the positive are frequent: integer rows in
    {-3..3} at D = 384 spread the scores of a row over a few hundred integers, and 4096 keys share them."""
    g = np.random.default_rng(4096 * 7 + 4096 * 3 + 384)                               # integer_rows(4096, 4096, 384) there
    q = g.integers(-3, 4, (4096, 384)).astype(np.float32)
    k = g.integers(-3, 4, (4096, 384)).astype(np.float32)
    S = (q.astype(np.float64) @ k.astype(np.float64).T).astype(np.int64)
    assert ((S == np.diagonal(S)[:, None]).sum(1) > 1).mean() > 0.9
