"""CPU checks of the probe block of the pan-organ evaluation: the host-side validation of the two library entries, the argument checking of
``ops.gram`` / ``ops.softmax_probe``, and ``dinox.probes`` (series split, L-BFGS fit, AUC, bootstrap, ridge, statistics) with the two
kernels replaced by float64 NumPy stand-ins, against the results the real reference recorded in tests/golden/panorgan_probes.npz.
No kernel is launched."""
import importlib.util
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

SCRIPT = os.path.join(ROOT, "dino-x_amd", "scripts", "evaluate_panorgan.py")


# ------------------------------------------------------------------------------------------ float64 stand-ins of the kernels
def host_gram(x, shift=None):
    z = x.cpu().numpy().astype(np.float64)
    if shift is not None:
        z = z - shift.cpu().numpy().astype(np.float64)
    return torch.from_numpy(z.T @ z), torch.from_numpy(z.sum(0))


def host_softmax_probe(x, label, theta, *, want_grad=True, want_prob=False):
    X = np.concatenate([x.cpu().numpy().astype(np.float64), np.ones((x.shape[0], 1))], 1)
    th, y = theta.cpu().numpy().astype(np.float64), label.cpu().numpy()
    z = X @ th.T
    m = z.max(1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(z - m).sum(1))
    p = np.exp(z - lse[:, None])
    ok = (y >= 0) & (y < th.shape[0])
    onehot = np.zeros_like(p)
    onehot[np.nonzero(ok)[0], y[ok]] = 1.0
    loss = float((lse - (z * onehot).sum(1))[ok].sum())
    grad = ((p - onehot) * ok[:, None]).T @ X
    return (torch.tensor(loss, dtype=torch.float64) if want_grad else None, torch.from_numpy(grad) if want_grad else None,
            torch.from_numpy(p.astype(np.float32)) if want_prob else None)


@pytest.fixture
def probes(monkeypatch):
    from dinox import ops, probes
    monkeypatch.setattr(ops, "gram", host_gram)
    monkeypatch.setattr(ops, "softmax_probe", host_softmax_probe)
    return probes


@pytest.fixture(scope="module")
def script():
    spec = importlib.util.spec_from_file_location("evaluate_panorgan_probes", SCRIPT)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_fixture():
    z = np.load(os.path.join(GOLDEN, "panorgan_probes.npz"))
    names = [str(s) for s in z["label_names"]]
    ref = {k: json.loads(str(z[f"reference_{k}"])) for k in ("probe", "ridge", "stats")}
    return z, torch.from_numpy(z["rows"]), [names[i] for i in z["labels"]], [str(s) for s in z["series"]], z["spacings"], ref


# ------------------------------------------------------------------------------------------ library entries, host side
def test_entries_validate_arguments_on_the_host():
    from dinox import _lib
    L = _lib.lib
    assert L.dinox_gram_ws_bytes(0, 8) == 0 and L.dinox_gram_ws_bytes(4, 0) == 0 and L.dinox_gram_ws_bytes(4, 1025) == 0
    assert L.dinox_gram_ws_bytes(1, 1) == (128 * 128 + 128) * 4                      # one tile, one split
    b = L.dinox_gram_ws_bytes(65536, 385)                                            # 4 panels: 10 upper tiles, at most 512 workgroups
    assert b % ((10 * 128 * 128 + 4 * 128) * 4) == 0 and 1 <= b // ((10 * 128 * 128 + 4 * 128) * 4) <= 52
    assert L.dinox_gram_ws_bytes(65536, 385) == b                                    # pure in the sizes
    for args, word in (((None, 8, 4, 8, None, 16, 16, 16, None), "null pointer"), ((16, 8, 4, 8, None, None, 16, 16, None), "null pointer"),
                       ((16, 8, 4, 8, None, 16, 16, None, None), "null pointer"), ((16, 8, 4, 0, None, 16, 16, 16, None), "D=0"),
                       ((16, 1025, 4, 1025, None, 16, 16, 16, None), "D=1025"), ((16, 7, 4, 8, None, 16, 16, 16, None), "ldx=7"),
                       ((16, 8, 0, 8, None, 16, 16, 16, None), "N=0")):
        assert L.dinox_gram_f32(*args) == -1 and word in _lib.last_error(), args
    P = L.dinox_softmax_probe_ws_bytes
    assert P(0, 8, 3) == 0 and P(4, 0, 3) == 0 and P(4, 1025, 3) == 0 and P(4, 8, 1) == 0 and P(4, 8, 33) == 0
    assert P(1, 1, 2) == 8 + 2 * 2 * 4 and P(65536, 384, 8) == 512 * (8 + 8 * 385 * 4)
    ok = dict(x=16, ldx=8, label=16, N=4, D=8, C=3, theta=16, loss=16, grad=16, prob=16, ws=16, stream=None)
    for change, word in ((dict(x=None), "null pointer"), (dict(label=None), "null pointer"), (dict(theta=None), "null pointer"),
                         (dict(ws=None), "null pointer"), (dict(loss=None, grad=None, prob=None), "null pointer"), (dict(C=1), "C=1"),
                         (dict(C=33), "C=33"), (dict(D=0), "D=0"), (dict(D=1025, ldx=1025), "D=1025"), (dict(ldx=7), "ldx=7"), (dict(N=0), "N=0")):
        a = dict(ok, **change)
        assert L.dinox_softmax_probe(*a.values()) == -1 and word in _lib.last_error(), change


def test_ops_argument_errors_without_a_device():
    from dinox import ops
    x = torch.zeros(6, 8)
    with pytest.raises(ValueError, match=r"gram: fp32 \[N, D\].*\(6, 8\)"):
        ops.gram(x.double())
    with pytest.raises(ValueError, match="gram: fp32"):
        ops.gram(x[0])
    with pytest.raises(ValueError, match="D=1025"):
        ops.gram(torch.zeros(2, 1025))
    with pytest.raises(ValueError, match="N=0"):
        ops.gram(torch.zeros(0, 8))
    with pytest.raises(ValueError, match=r"shift must be fp32 of shape \(8,\)"):
        ops.gram(x, torch.zeros(7))
    with pytest.raises(ValueError, match="shift must be fp32"):
        ops.gram(x, torch.zeros(8, dtype=torch.float64))
    with pytest.raises(ValueError, match="rows on cpu, shift on meta"):
        ops.gram(x, torch.zeros(8, device="meta"))
    y, th = torch.zeros(6, dtype=torch.int64), torch.zeros(3, 9)
    with pytest.raises(ValueError, match="softmax_probe: fp32"):
        ops.softmax_probe(x.bfloat16(), y, th)
    with pytest.raises(ValueError, match=r"theta must be fp32 \[C, 9\]"):
        ops.softmax_probe(x, y, torch.zeros(3, 8))
    for C in (1, 33):
        with pytest.raises(ValueError, match=r"C must lie in \[2, 32\]"):
            ops.softmax_probe(x, y, torch.zeros(C, 9))
    with pytest.raises(ValueError, match=r"label must be int32 or int64 of shape \(6,\)"):
        ops.softmax_probe(x, y[:5], th)
    with pytest.raises(ValueError, match="label must be int32 or int64"):
        ops.softmax_probe(x, y.float(), th)
    with pytest.raises(ValueError, match="nothing asked for"):
        ops.softmax_probe(x, y, th, want_grad=False)
    with pytest.raises(ValueError, match="D=1025"):
        ops.softmax_probe(torch.zeros(2, 1025), y[:2], torch.zeros(3, 1026))
    # well-formed calls on host tensors reach the device check: there is no CPU path
    for call in (lambda: ops.gram(x), lambda: ops.gram(x, torch.zeros(8)), lambda: ops.softmax_probe(x, y, th),
                 lambda: ops.softmax_probe(x, y.int(), th, want_grad=False, want_prob=True)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


# ------------------------------------------------------------------------------------------ the launch plans, mirrored
# Which template instantiation a call runs cannot be seen from Python, but the plans are pure functions of the sizes.  These are
# csrc/gram.hip (gram_plan, the VEC predicate) and csrc/probe.hip (pb_groups, pb_lds_bytes, the nb -> NB dispatch, the VEC predicate) again;
# the shape lists below are the ones tests/test_probes_gpu.py runs, each with the plan facts it is in the list for.
def cdiv(a, b):
    return -(-a // b)


def rows_are_vec(ld, D, off):
    """16-byte row loads: the base 16-byte aligned (the buffer is, so the column offset decides) and a pitch of whole quads."""
    return off % 4 == 0 and (ld or D) % 4 == 0


def gram_plan(N, D, ld=0, off=0):
    T = cdiv(D, 128)
    tiles = T * (T + 1) // 2
    slabs = cdiv(N, 16)
    per = cdiv(slabs, min(cdiv(512, tiles), slabs))
    splits = cdiv(slabs, per)
    return dict(T=T, tiles=tiles, splits=splits, slabs=per, last_split_slabs=slabs - (splits - 1) * per, last_slab_rows=N - (slabs - 1) * 16,
                vec=rows_are_vec(ld, D, off), ws_bytes=splits * (tiles * 128 * 128 + T * 128) * 4)


def probe_plan(N, D, C, ld=0, off=0):
    blocks = cdiv(N, 32)
    groups = min(blocks, 512)
    nb = cdiv(D, 128)
    colsz = cdiv(D, 4) * 4
    pitch = (colsz - 4 + 63) // 64 * 64 + 4
    return dict(blocks=blocks, groups=groups, last_block_rows=N - (blocks - 1) * 32, nb=nb, NB=nb if nb <= 4 else 8,
                lds_bytes=(32 * pitch + 4 * 32 * 33 + 32 * 36 + 32) * 4, vec=rows_are_vec(ld, D, off), ws_bytes=groups * (8 + C * (D + 1) * 4))


# ((N, D, ld, column offset), the facts the case exists for).  ld = 0: contiguous rows.
GRAM_PATHS = [
    ((300, 1024, 0, 0), dict(T=8, tiles=36, vec=True, splits=10, slabs=2)),                        # ViT-L: the whole 8 x 8 triangle
    ((700, 768, 0, 0), dict(T=6, tiles=21, vec=True, splits=22, slabs=2)),                         # ViT-B
    ((300, 1023, 0, 0), dict(T=8, tiles=36, vec=False, splits=10, slabs=2)),                       # odd pitch; the last panel 127 wide
    ((2000, 384, 0, 0), dict(T=3, tiles=6, vec=True, splits=63, slabs=2, last_split_slabs=1)),     # the statistics shape; a short last split
    ((8300, 64, 0, 0), dict(T=1, tiles=1, vec=True, splits=260, slabs=2, last_slab_rows=12)),      # one tile; a ragged last slab
    ((1030, 130, 132, 0), dict(T=2, tiles=3, vec=True, last_slab_rows=6)),                         # a quad across D; a panel 2 columns wide
    ((513, 64, 80, 1), dict(T=1, vec=False)),                                                      # whole-quad pitch, base one float off
]
GRAM_PATH_SHAPES = [s for s, _ in GRAM_PATHS]
GRAM_PATTERN_SHAPE = (300, 1024)                                # x[i, j] = (j % 7) - 3 on every row: plan of GRAM_PATHS[0]

# ((N, D, C, span), facts) for the contiguous cases, ((N, D, C, ld, column offset), facts) for rows of a wider buffer
PROBE_PATHS = [
    ((70, 385, 3, 8.0), dict(NB=4, nb=4, vec=False)),                                              # the lowest NB = 4, odd pitch
    ((70, 512, 32, 8.0), dict(NB=4, nb=4, vec=True)),                                              # NB = 4 full, all 32 classes
    ((70, 513, 5, 8.0), dict(NB=8, nb=5, vec=False)),                                              # three idle 128-column blocks
    ((45, 768, 7, 8.0), dict(NB=8, nb=6, vec=True)),                                               # ViT-B
    ((45, 1024, 32, 8.0), dict(NB=8, nb=8, vec=True, lds_bytes=153216)),                           # ViT-L: the largest footprint
    ((45, 1024, 32, 60.0), dict(NB=8, nb=8, vec=True, lds_bytes=153216)),
    ((16384, 7, 3, 8.0), dict(blocks=512, groups=512)),                                            # the last size with one trip
    ((16385, 7, 3, 8.0), dict(blocks=513, groups=512, last_block_rows=1)),                         # one workgroup takes a second block
    ((16421, 7, 3, 8.0), dict(blocks=514, groups=512, last_block_rows=5)),                         # two do; the last block has 5 rows
    ((16421, 520, 4, 8.0), dict(blocks=514, groups=512, NB=8, nb=5, vec=True)),                    # the walk on NB = 8
]
PROBE_PATH_SHAPES = [s for s, _ in PROBE_PATHS]
PROBE_PITCH_PATHS = [
    ((70, 66, 5, 68, 0), dict(NB=1, vec=True)),                                                    # VEC, the last quad straddles D
    ((70, 64, 5, 68, 1), dict(NB=1, vec=False)),                                                   # whole-quad pitch, base one float off
]
PROBE_PITCH_SHAPES = [s for s, _ in PROBE_PITCH_PATHS]
LDS_LIMIT = 160 * 1024                                          # per workgroup on gfx950


def holds(plan, facts):
    return {k: plan[k] for k in facts} == facts


def test_gram_shapes_reach_the_paths_they_are_named_for():
    from dinox import _lib
    for (N, D, ld, off), facts in GRAM_PATHS:
        plan = gram_plan(N, D, ld, off)
        assert _lib.lib.dinox_gram_ws_bytes(N, D) == plan["ws_bytes"], (N, D)
        assert holds(plan, facts), ((N, D, ld, off), plan)
        assert 25 * N < 2 ** 24                                                          # the integer test's exactness condition
    plans = {s: gram_plan(*s) for s in GRAM_PATH_SHAPES}
    assert sum(p["T"] == 8 for p in plans.values()) >= 2 and any(p["T"] == 6 for p in plans.values())
    multi = [s for s, p in plans.items() if p["splits"] >= 2 and p["slabs"] >= 2]          # the prefetch-under-products loop
    assert any(plans[s]["vec"] and plans[s]["tiles"] > 1 for s in multi) and any(not plans[s]["vec"] for s in multi)
    assert any(p["vec"] and s[1] % 4 for s, p in plans.items())                            # VEC with D % 4 != 0: the ragged quad
    assert any(not p["vec"] and (s[2] or s[1]) % 4 == 0 for s, p in plans.items())         # non-VEC through the base pointer alone
    assert holds(gram_plan(*GRAM_PATTERN_SHAPE), GRAM_PATHS[0][1])
    # the mirror is the library's plan elsewhere too: the shapes of the older tests and the limits
    for N, D in ((1, 1), (33, 7), (257, 65), (1000, 129), (4099, 385), (513, 64), (65536, 385), (65536, 1024), (15, 1024), (16, 128), (17, 129)):
        assert _lib.lib.dinox_gram_ws_bytes(N, D) == gram_plan(N, D)["ws_bytes"], (N, D)


def test_probe_shapes_reach_the_paths_they_are_named_for():
    from dinox import _lib
    P = _lib.lib.dinox_softmax_probe_ws_bytes
    plans = {}
    for (N, D, C, _), facts in PROBE_PATHS:
        plans[(N, D, C, 0, 0)] = plan = probe_plan(N, D, C)
        assert holds(plan, facts), ((N, D, C), plan)
    for (N, D, C, ld, off), facts in PROBE_PITCH_PATHS:
        plans[(N, D, C, ld, off)] = plan = probe_plan(N, D, C, ld, off)
        assert holds(plan, facts), ((N, D, C, ld, off), plan)
    for (N, D, C, _, _), plan in plans.items():
        assert P(N, D, C) == plan["ws_bytes"], (N, D, C)
        assert plan["lds_bytes"] <= LDS_LIMIT and D <= 128 * plan["NB"]
    assert {p["NB"] for p in plans.values()} == {1, 4, 8}                                  # NB = 1, 2, 3: PROBE_SHAPES of the GPU file
    assert {p["nb"] for p in plans.values() if p["NB"] == 8} >= {5, 6, 8}
    assert max(p["lds_bytes"] for p in plans.values()) == probe_plan(1, 1024, 2)["lds_bytes"]          # the largest any call can ask for
    walk = [s for s, p in plans.items() if p["blocks"] > p["groups"]]
    assert any(plans[s]["NB"] == 8 for s in walk) and any(plans[s]["NB"] == 1 for s in walk)
    assert any(p["blocks"] == p["groups"] == 512 for p in plans.values())
    assert any(p["vec"] and s[1] % 4 for s, p in plans.items())                            # VEC with D % 4 != 0
    assert any(not p["vec"] and (s[3] or s[1]) % 4 == 0 for s, p in plans.items())         # non-VEC through the base pointer alone
    for N, D, C in ((1, 1, 2), (67, 7, 3), (300, 65, 10), (1031, 384, 32), (2050, 129, 5), (65536, 384, 8), (16384, 1024, 32), (16385, 1024, 32)):
        assert P(N, D, C) == probe_plan(N, D, C)["ws_bytes"], (N, D, C)


# ------------------------------------------------------------------------------------------ series split
def test_series_split_matches_the_reference_and_hand_cases():
    from dinox.probes import series_split
    z, _, labels, series, _, ref = load_fixture()
    sp = series_split(labels, series, 42)
    assert np.array_equal(sp.train_idx, z["train_idx"]) and np.array_equal(sp.test_idx, z["test_idx"])      # the rows the reference's classifier saw
    assert len(sp.train_idx) == ref["probe"]["train_slices"] == ref["ridge"]["train_slices"]
    assert len(sp.test_idx) == ref["probe"]["test_slices"] and len(sp.train_series) == ref["probe"]["train_series"]
    assert len(sp.test_series) == ref["probe"]["test_series"]
    # a one-series dataset is all train; 2 series -> 1 / 1; 4 series -> int(3.2) = 3 / 1; 5 series: int(4.0) = 4 / 1
    lab = ["a"] * 3 + ["b"] * 4 + ["c"] * 8 + ["d"] * 5
    ser = ["a0"] * 3 + ["b0", "b0", "b1", "b1"] + [f"c{i // 2}" for i in range(8)] + [f"d{i}" for i in range(5)]
    sp = series_split(lab, ser, 7)
    in_train = lambda prefix: sum(s.startswith(prefix) for s in sp.train_series)
    in_test = lambda prefix: sum(s.startswith(prefix) for s in sp.test_series)
    assert (in_train("a"), in_test("a")) == (1, 0) and (in_train("b"), in_test("b")) == (1, 1)
    assert (in_train("c"), in_test("c")) == (3, 1) and (in_train("d"), in_test("d")) == (4, 1)
    assert sorted(sp.train_idx.tolist() + sp.test_idx.tolist()) == list(range(20)) and list(sp.train_idx) == sorted(sp.train_idx)
    assert series_split(lab, ser, 7).train_series == sp.train_series                                        # a function of the seed
    # the dataset of a series is the dataset of its LAST row; None -> "unknown"
    sp = series_split(["x", "y", None, None], ["s", "s", "t", "u"], 0)
    assert sp.dataset_of == {"s": "y", "t": "unknown", "u": "unknown"}
    with pytest.raises(ValueError, match="3 labels but 2 series"):
        series_split(["a"] * 3, ["s"] * 2, 0)


# ------------------------------------------------------------------------------------------ host metrics
def test_rank_auc_counts_ties_as_half():
    from dinox.probes import probe_auc, rank_auc
    s, pos = np.array([0.1, 0.4, 0.4, 0.8, 0.4, 0.9]), np.array([False, False, True, True, False, True])
    pairs = [(a, b) for a in s[pos] for b in s[~pos]]
    want = sum(1.0 if a > b else (0.5 if a == b else 0.0) for a, b in pairs) / len(pairs)
    assert abs(rank_auc(s, pos) - want) <= 1e-15 and want == (1 + 0.5 + 0.5 + 3 + 3) / 9.0
    assert rank_auc(np.arange(4.0), np.array([0, 0, 1, 1], bool)) == 1.0 and np.isnan(rank_auc(s, np.zeros(6, bool)))
    p = np.array([[0.7, 0.2, 0.1], [0.1, 0.8, 0.1], [0.2, 0.2, 0.6], [0.5, 0.4, 0.1]])
    y = np.array([0, 1, 2, 1])
    assert abs(probe_auc(p, y) - np.mean([rank_auc(p[:, c], y == c) for c in range(3)])) <= 1e-15
    assert probe_auc(p[:, :2], np.array([0, 1, 1, 0])) == rank_auc(p[:, 1], np.array([0, 1, 1, 0], bool))


def test_lbfgs_minimises_a_quadratic_and_stops_at_resolution():
    from dinox.probes import lbfgs_minimize
    g = np.random.default_rng(0)
    M = g.standard_normal((12, 12))
    A, b = M @ M.T + np.eye(12), g.standard_normal(12)
    x, f, grad, evals, reason = lbfgs_minimize(lambda v: (0.5 * v @ A @ v - b @ v, A @ v - b), np.zeros(12), 1.0, gtol=1e-6)
    assert reason == "gtol" and np.abs(x - np.linalg.solve(A, b)).max() <= 1e-6 and evals < 200          # |x - x*| <= |g| / lambda_min, lambda_min >= 1
    # a function evaluated at the fp32 rounding of its argument: the search ends when no step lowers it, without spending the budget
    r = lambda v: v.astype(np.float32).astype(np.float64)
    x, f, grad, evals, reason = lbfgs_minimize(lambda v: (0.5 * r(v) @ A @ r(v) - b @ r(v), A @ r(v) - b), np.zeros(12), 1.0, gtol=1e-30)
    assert reason == "resolution" and evals < 2000 and np.abs(x - np.linalg.solve(A, b)).max() <= 1e-5


# ------------------------------------------------------------------------------------------ the three metrics against the reference's record
def test_logistic_probe_reproduces_the_reference(probes):
    z, rows, labels, series, _, ref = load_fixture()
    want = ref["probe"]
    got = probes.logistic_probe(rows, labels, series, seed=42, return_details=True)
    prob, fit = got.pop("probabilities"), got.pop("fit")
    print(f"fit: {fit}; max |p - prob_tight| = {np.abs(prob - z['prob_tight']).max():.3e}; auc {got['auc']:.9f} tight {float(z['auc_tight']):.9f} "
          f"reference {want['auc']:.9f}")
    assert list(got) == list(want)
    for key in ("labels", "train_series", "test_series", "train_slices", "test_slices", "note", "accuracy", "accuracy_ci95"):
        assert got[key] == want[key], key                       # predictions are the reference's by the fixture's margin: exact
    slack = float(z["auc_slack"])
    assert abs(got["auc"] - float(z["auc_tight"])) <= slack + 1e-12
    assert abs(got["auc"] - want["auc"]) <= slack + abs(want["auc"] - float(z["auc_tight"])) + 1e-12
    # float64 stand-in, both fits at the optimum of one objective: the distance is the two optimisers' stopping error (the fp32 probabilities
    # of the stand-in carry 6e-8)
    assert np.abs(prob - z["prob_tight"]).max() <= 1e-5
    assert fit["stopped_by"] in ("gtol", "resolution") and fit["evaluations"] <= 2000


def test_logistic_probe_error_dicts(probes):
    x = torch.zeros(4, 3)
    assert probes.logistic_probe(x, ["a"] * 4, ["s"] * 4) == {"error": "insufficient series for train/test split"}
    assert probes.logistic_probe(x, ["a"] * 4, ["s", "s", "t", "t"]) == {"error": "need at least 2 datasets in both train and test splits"}
    with pytest.raises(ValueError, match="4 embeddings but 3 labels"):
        probes.logistic_probe(x, ["a"] * 3, ["s"] * 4)


def test_spacing_ridge_reproduces_the_reference(probes):
    _, rows, labels, series, spacings, ref = load_fixture()
    want = ref["ridge"]
    for sp in (spacings, torch.from_numpy(spacings), spacings[:, 0]):
        got = probes.spacing_ridge(rows, sp, labels, series, seed=42)
        assert list(got) == list(want)
        for key in ("target", "train_slices", "test_slices", "note"):
            assert got[key] == want[key]
        print(f"r2 {got['r2']:.9f} vs {want['r2']:.9f}, mae {got['mae_log_spacing']:.9f} vs {want['mae_log_spacing']:.9f}")
        assert abs(got["r2"] - want["r2"]) <= 1e-5 and abs(got["mae_log_spacing"] - want["mae_log_spacing"]) <= 1e-5
    assert probes.spacing_ridge(rows[:4], spacings[:4], ["a"] * 4, ["s"] * 4) == {"error": "insufficient series for split"}
    with pytest.raises(ValueError, match="spacings must be"):
        probes.spacing_ridge(rows, spacings[:-1], labels, series)


def test_embedding_stats_reproduces_the_reference(probes):
    _, rows, labels, _, spacings, ref = load_fixture()
    want = ref["stats"]
    got = probes.embedding_stats(rows, spacings, labels)
    assert list(got) == list(want) and list(got["per_dataset"]) == list(want["per_dataset"])
    for name, w in want["per_dataset"].items():
        g = got["per_dataset"][name]
        assert list(g) == list(w) and g["n"] == w["n"]
        assert abs(g["embedding_std"] - w["embedding_std"]) <= 1e-6 and abs(g["intra_cosine_to_centroid"] - w["intra_cosine_to_centroid"]) <= 1e-6
        assert abs(abs(g["pca1_spacing_correlation"]) - abs(w["pca1_spacing_correlation"])) <= 1e-5
    assert list(got["cross_dataset_centroid_cosine"]) == list(want["cross_dataset_centroid_cosine"])
    for pair, w in want["cross_dataset_centroid_cosine"].items():
        assert abs(got["cross_dataset_centroid_cosine"][pair] - w) <= 1e-6
    # the rows in any order give the same numbers (they are sorted by dataset inside); n <= 2 has no principal axis
    perm = np.random.default_rng(0).permutation(len(labels))
    again = probes.embedding_stats(rows[perm], spacings[perm], [labels[i] for i in perm])
    for name, g in got["per_dataset"].items():
        for key, v in g.items():
            assert abs(again["per_dataset"][name][key] - v) <= 1e-9
    tiny = probes.embedding_stats(rows[:5], np.array([0.5, 0.6, 0.7, 0.9, 0.8]), ["p", "p", "q", "q", "q"])
    assert np.isnan(tiny["per_dataset"]["p"]["pca1_spacing_correlation"]) and np.isfinite(tiny["per_dataset"]["q"]["pca1_spacing_correlation"])
    assert list(tiny["cross_dataset_centroid_cosine"]) == ["p_vs_q"]


# ------------------------------------------------------------------------------------------ script
def test_script_probe_flags(script):
    ap = script.build_parser(probe_flags=True)
    have = {s for a in ap._actions for s in a.option_strings if s.startswith("--")} - {"--help"}
    plain = {s for a in script.build_parser()._actions for s in a.option_strings if s.startswith("--")} - {"--help"}
    assert have - plain == {"--probes", "--skip-probes"}
    d = vars(ap.parse_args(["--checkpoint", "x.pth"]))
    assert d["probes"] is False and d["skip_probes"] is False
    d = vars(ap.parse_args(["--checkpoint", "x.pth", "--probes", "--skip-probes"]))
    assert d["probes"] is True and d["skip_probes"] is True
    with pytest.raises(SystemExit):
        script.build_parser().parse_args(["--checkpoint", "x.pth", "--probes"])


def test_script_probe_series_and_output(script, probes, capsys):
    class Row:
        def __init__(self, series_dir, dataset):
            self.series_dir, self.dataset = series_dir, dataset

    rows = [Row("series0000", "synthetic_a"), Row("series0000", "synthetic_b")]
    assert script.probe_series(rows, True) == ["series0000:synthetic_a", "series0000:synthetic_b"]
    assert script.probe_series(rows, False) == ["series0000", "series0000"]
    _, E, labels, series, spacings, ref = load_fixture()
    metrics = {"domain_clustering": 1}
    script.run_probes(E, torch.from_numpy(spacings), labels, series, 42, metrics)
    assert list(metrics) == ["domain_clustering", "dataset_discrimination_probe", "spacing_prediction", "embedding_stats"]
    out = capsys.readouterr().out.splitlines()
    p, r = metrics["dataset_discrimination_probe"], metrics["spacing_prediction"]
    assert f"  Accuracy: {p['accuracy']:.3f} (CI: {p['accuracy_ci95']})" in out and f"  AUC: {p['auc']:.3f}" in out
    assert f"  R²: {r['r2']:.3f}" in out and f"  MAE(log spacing): {r['mae_log_spacing']:.4f}" in out
    assert sum(line.startswith("  Cross: ") for line in out) == 3 and any(line.startswith("  abdomen_ct: std=") for line in out)
    json.dumps(metrics)                                          # plain Python numbers all the way down
