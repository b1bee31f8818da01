"""CPU checks of the pan-organ evaluation's view metrics (metric 1, per-dataset view retrieval; metric 3, spacing counterfactual): the
opt-in flag group of scripts/evaluate_panorgan.py and the host-side summaries of dinox/retrieval.py against results recorded from the
reference's own functions (tests/golden/panorgan_views.npz, written by tests/golden/make_golden_views.py).  No kernel is launched."""
import importlib.util
import json
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

SCRIPT = os.path.join(ROOT, "dino-x_amd", "scripts", "evaluate_panorgan.py")
VIEW_FLAGS = {"--view-metrics": False, "--n-retrieval": 512, "--n-counterfactual": 256, "--skip-view-retrieval": False}


@pytest.fixture(scope="module")
def script():
    spec = importlib.util.spec_from_file_location("evaluate_panorgan_views_cpu", SCRIPT)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "panorgan_views.npz"))


def stable_ranks(S, target):
    """#{j : S[i,j] > S[i,t_i]} + #{j < t_i : S[i,j] == S[i,t_i]} (tests/test_retrieval_gpu.py)."""
    pos = S[np.arange(S.shape[0]), target][:, None]
    before = np.arange(S.shape[1])[None, :] < target[:, None]
    return ((S > pos) | ((S == pos) & before)).sum(1)


def same_dict(got, want, tol=1e-12):
    """Equal keys in equal order, recursively; numbers within tol, everything else exactly."""
    assert list(got) == list(want), (list(got), list(want))
    for key in want:
        g, w = got[key], want[key]
        if isinstance(w, dict):
            same_dict(g, w, tol)
        elif isinstance(w, float):
            assert isinstance(g, float) and abs(g - w) <= tol, (key, g, w)
        else:
            assert type(g) is type(w) and g == w, (key, g, w)


def flags(ap):
    return {s: a.default for a in ap._actions for s in a.option_strings if s.startswith("--") and s != "--help"}


def test_view_flag_group_is_exactly_the_four_new_flags(script):
    with_views, without = flags(script.build_parser(probe_flags=True, view_flags=True)), flags(script.build_parser(probe_flags=True))
    assert {f: with_views[f] for f in set(with_views) - set(without)} == VIEW_FLAGS
    assert {f: with_views[f] for f in without} == without                       # nothing else moved
    assert flags(script.build_parser(view_flags=True)).keys() - flags(script.build_parser()).keys() == set(VIEW_FLAGS)
    d = vars(script.build_parser(probe_flags=True, view_flags=True).parse_args(["--checkpoint", "x.pth", "--view-metrics", "--n-retrieval", "7"]))
    assert d["view_metrics"] is True and d["n_retrieval"] == 7 and d["n_counterfactual"] == 256 and d["skip_view_retrieval"] is False
    for ap in (script.build_parser(), script.build_parser(probe_flags=True)):
        for flag in VIEW_FLAGS:
            with pytest.raises(SystemExit):
                ap.parse_args(["--checkpoint", "x.pth", flag] + (["3"] if flag.startswith("--n-") else []))


def test_per_dataset_metrics_match_the_reference(golden):
    from dinox.retrieval import per_dataset_metrics_from_ranks
    names = [str(n) for n in golden["names"]]
    want = json.loads(str(golden["reference_retrieval"]))
    D = golden["Q_0"].shape[1]
    ranks, sizes = [], []
    for g in range(len(names)):
        S = golden[f"Q_{g}"].astype(np.float64) @ golden[f"K_{g}"].astype(np.float64).T
        # the fixture's promise: no key within 2 D 2^-23 of the positive, so the fp32 product of the reference saw the same order
        off = np.abs(S - np.diagonal(S)[:, None])
        np.fill_diagonal(off, np.inf)
        assert off.min() > 2.0 * D * 2.0 ** -23
        ranks.append(stable_ranks(S, np.arange(S.shape[0])))
        sizes.append(S.shape[0])
    assert len(set(sizes)) > 1 and min(sizes) < int(golden["n_per_dataset"]) == max(sizes)
    got = per_dataset_metrics_from_ranks(np.concatenate(ranks), sizes, names, topk=int(golden["topk"]))
    same_dict(got, want)
    assert all(0.0 < want[n]["top1"] < 1.0 for n in names)                     # a wrong rank can move it
    # names are sorted whatever order the groups come in; int32 ranks (the kernel's) are taken
    back = per_dataset_metrics_from_ranks(np.concatenate(ranks[::-1]).astype(np.int32), sizes[::-1], names[::-1], topk=int(golden["topk"]))
    same_dict(back, want)
    assert "passed" not in got[names[0]]
    with pytest.raises(ValueError):
        per_dataset_metrics_from_ranks(np.zeros(5), [2, 2], ["a", "b"])
    with pytest.raises(ValueError):
        per_dataset_metrics_from_ranks(np.zeros(4), [2, 2], ["a", "b"], topk=0)


def test_sampling_reproduces_the_reference_picks(golden):
    from dinox.retrieval import per_dataset_picks
    labels = [str(d) for d in golden["datasets"]]
    names, picks = per_dataset_picks(labels, int(golden["n_per_dataset"]), int(golden["seed"]))
    assert names == [str(n) for n in golden["names"]]
    for g, name in enumerate(names):
        rows = [i for i, d in enumerate(labels) if d == name]                  # the dataset's rows in index order
        assert picks[g] == [rows[j] for j in golden[f"picks_{g}"]], name
        assert len(picks[g]) == min(int(golden["n_per_dataset"]), len(rows))
    # unlabelled rows form the dataset "unknown"
    names, picks = per_dataset_picks(["b", None, "a", "", "b"], 2, 0)
    assert names == ["a", "b", "unknown"] and picks[0] == [2] and sorted(picks[1]) == [0, 4] and sorted(picks[2]) == [1, 3]


def test_counterfactual_summary_matches_the_reference(golden):
    from dinox.retrieval import counterfactual_summary
    want = json.loads(str(golden["reference_counterfactual"]))
    got = counterfactual_summary(golden["d_real_2x"], golden["d_real_half"], golden["d_half_2x"])
    same_dict(got, want)
    assert got["interpretation"] == want["interpretation"] and got["n"] == int(golden["n_counterfactual"])
    assert want["cosine_distance_real_vs_2x"]["mean"] > 1e-3                   # the recorded model does read its spacing
    same_dict(counterfactual_summary(*(list(golden[k]) for k in ("d_real_2x", "d_real_half", "d_half_2x"))), want)
    with pytest.raises(ValueError):
        counterfactual_summary([0.1], [0.1, 0.2], [0.1])


def test_new_entries_validate_arguments_on_the_host():
    """Argument validation happens before any launch: safe without a GPU."""
    import torch
    from dinox import _lib, ops
    L = _lib.lib
    assert L.dinox_retrieval_rank_windowed_ws_bytes(0, 4, 8) == 0
    for n in (1, 852, 2560, 8192, 200000):
        b = L.dinox_retrieval_rank_windowed_ws_bytes(n, n, 384)
        assert b % (12 * n) == 0 and 1 <= b // (12 * n) <= 4, (n, b)          # O(Nq), never O(Nq x Nk)
    rc = L.dinox_retrieval_rank_windowed(None, 8, None, 8, None, None, None, 4, 4, 8, None, None, None, None, None, None)
    assert rc == -1 and "null pointer" in _lib.last_error()
    rc = L.dinox_retrieval_rank_windowed(16, 8, 16, 8, None, 16, 16, 4, 5, 8, 16, 16, 16, 16, 16, None)
    assert rc == -1 and "Nq == Nk" in _lib.last_error()
    rc = L.dinox_retrieval_rank_windowed(16, 4, 16, 8, 16, 16, 16, 4, 5, 8, 16, 16, 16, 16, 16, None)
    assert rc == -1 and "ldq" in _lib.last_error()
    rc = L.dinox_row_dots(None, 8, None, 8, 4, 8, None, None)
    assert rc == -1 and "null pointer" in _lib.last_error()
    rc = L.dinox_row_dots(16, 4, 16, 8, 4, 8, 16, None)
    assert rc == -1 and "lda" in _lib.last_error()
    z, w = torch.zeros(4, 8), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.retrieval_rank_windowed(z, z, w, w)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.row_dots(z, z)
