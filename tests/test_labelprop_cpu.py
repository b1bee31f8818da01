"""CPU checks of dense label propagation: the argument checking of ``ops.label_propagate`` and of the library entry (host-side, nothing
is launched), ``dinox.propagate``'s soft labels and schedule against the float64 oracle, the script's parser and synthetic case, the
oracle's own identities, and the input conditions that the GPU float cases rely on -- asserted here on the float64 reference alone."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

import _labelprop_oracle as O
from conftest import ROOT

SCRIPT = os.path.join(ROOT, "dino-x_amd", "scripts", "propagate_volume.py")


@pytest.fixture(scope="module")
def script():
    spec = importlib.util.spec_from_file_location("propagate_volume", SCRIPT)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------------------------------ ops.label_propagate argument checking
def test_label_propagate_argument_errors_without_a_device():
    from dinox import ops
    q, k, seg = torch.zeros(9, 8), torch.zeros(18, 8), torch.zeros(18, 3)
    with pytest.raises(ValueError, match=r"fp32 q \[N, D\].*bfloat16"):
        ops.label_propagate(q.bfloat16(), k, seg, 3)
    with pytest.raises(ValueError, match=r"fp32 q.*\(18, 7\)"):
        ops.label_propagate(q, torch.zeros(18, 7), seg, 3)                      # different D
    with pytest.raises(ValueError, match="fp32 q"):
        ops.label_propagate(q[0], k, seg, 3)                                    # not 2-D
    with pytest.raises(ValueError, match="fp32 q"):
        ops.label_propagate(q, k, torch.zeros(17, 3), 3)                        # seg rows != key rows
    with pytest.raises(ValueError, match="fp32 q"):
        ops.label_propagate(q, k, seg.numpy(), 3)
    with pytest.raises(ValueError, match=r"q has 9 rows.*g g = 16"):
        ops.label_propagate(q, k, seg, 4)
    with pytest.raises(ValueError, match="k has 20 rows"):
        ops.label_propagate(q, torch.zeros(20, 8), torch.zeros(20, 3), 3)
    with pytest.raises(ValueError, match="k has 0 rows"):
        ops.label_propagate(q, torch.zeros(0, 8), torch.zeros(0, 3), 3)
    for C in (1, 65):
        with pytest.raises(ValueError, match=rf"C = {C} classes, outside \[2, 64\]"):
            ops.label_propagate(q, k, torch.zeros(18, C), 3)
    for g in (0, -3, 3.0, True, None):
        with pytest.raises(ValueError, match="g must be an integer >= 1"):
            ops.label_propagate(q, k, seg, g)
    for K in (0, 33, -3, 2.0, True, None):
        with pytest.raises(ValueError, match=r"K must be an integer in \[1, 32\]"):
            ops.label_propagate(q, k, seg, 3, K=K)
    for r in (1.5, None, True, 1 << 31):
        with pytest.raises(ValueError, match="radius must be an integer"):
            ops.label_propagate(q, k, seg, 3, radius=r)
    for T in (0.0, -0.1, float("nan"), float("inf"), "0.1", True, 1e-45):
        with pytest.raises(ValueError, match="temperature"):
            ops.label_propagate(q, k, seg, 3, temperature=T)
    with pytest.raises(ValueError, match="q on cpu, k on meta"):
        ops.label_propagate(q, torch.zeros(18, 8, device="meta"), seg, 3)
    # a well-formed call on host tensors reaches the device check: there is no CPU path
    for kw in ({}, {"K": np.int64(2), "radius": -1}, {"K": 32, "radius": np.int32(40), "temperature": 1}):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.label_propagate(q, k, seg, 3, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.label_propagate(torch.zeros(9, 16)[:, :8], k, seg, 3)               # a strided row view


def test_labelprop_entry_validates_arguments_on_the_host():
    """Argument validation happens before any launch: safe without a GPU.  Every refusal names the offending value."""
    from dinox import _lib
    L = _lib.lib

    def call(q=16, ldq=8, k=16, ldk=8, seg=16, g=3, F=2, D=8, C=3, K=5, radius=1, inv_t=10.0, out=16, idx=16, val=16, ws=16):
        return L.dinox_labelprop(q, ldq, k, ldk, seg, g, F, D, C, K, radius, inv_t, out, idx, val, ws, None)

    for K in (0, 33, -1):
        assert call(K=K) == -1 and f"K={K}" in _lib.last_error()
    for C in (1, 65, 0):
        assert call(C=C) == -1 and f"C={C}" in _lib.last_error()
    for name in ("q", "k", "seg", "out", "idx", "val", "ws"):
        assert call(**{name: None}) == -1 and "null pointer" in _lib.last_error()
    for kw, word in (({"g": 0}, "g=0"), ({"F": 0}, "F=0"), ({"D": 0}, "D=0"), ({"g": -2}, "g=-2")):
        assert call(**kw) == -1 and word in _lib.last_error()
    assert call(ldq=7) == -1 and "ldq=7" in _lib.last_error()
    assert call(ldk=4) == -1 and "ldk=4" in _lib.last_error()
    for t, word in ((0.0, "inv_temperature=0"), (-2.0, "inv_temperature=-2"), (float("inf"), "inv_temperature=inf"), (float("nan"), "nan")):
        assert call(inv_t=t) == -1 and word in _lib.last_error().lower()
    assert call(g=46341, F=1) == -1 and "g=46341" in _lib.last_error()          # g g itself past the int range
    assert call(g=1000, F=2148) == -1 and "F=2148" in _lib.last_error()         # F g g past 2^31 - 129
    # the workspace: 8 K bytes per patch and key split, a pure function of (g, F); 0 for what the call refuses
    assert L.dinox_labelprop_ws_bytes(1, 1, 1, 2, 1) == 8
    for g, F, K in ((14, 1, 5), (28, 8, 5), (28, 8, 32), (9, 2, 1)):
        b, N = L.dinox_labelprop_ws_bytes(g, F, 384, 4, K), g * g
        assert b == L.dinox_knn_ws_bytes(N, F * N, 384, K) and b % (8 * K * N) == 0 and b >= 8 * K * N
        assert b == L.dinox_labelprop_ws_bytes(g, F, 7, 64, K)
    for bad in ((0, 1, 8, 3, 5), (3, 0, 8, 3, 5), (3, 1, 0, 3, 5), (3, 1, 8, 1, 5), (3, 1, 8, 65, 5), (3, 1, 8, 3, 0), (3, 1, 8, 3, 33),
                (46341, 1, 8, 3, 5), (1000, 2148, 8, 3, 5)):
        assert L.dinox_labelprop_ws_bytes(*bad) == 0, bad


# ------------------------------------------------------------------------------------------ dinox.propagate
def test_patch_soft_labels_against_the_oracle():
    from dinox.propagate import patch_soft_labels
    rng = np.random.default_rng(3)
    for S, patch, C in ((12, 4, 3), (14, 7, 2), (6, 1, 5), (15, 5, 64)):
        lab = rng.integers(0, C, (S, S)).astype(np.uint8)
        lab[rng.random((S, S)) < 0.2] = 255                                     # ignore
        lab[:patch, :patch] = 255                                               # an all-ignored patch
        got = patch_soft_labels(torch.from_numpy(lab), C, patch)
        want = O.patch_soft_labels(lab, C, patch)
        assert got.dtype == torch.float32 and tuple(got.shape) == ((S // patch) ** 2, C)
        assert np.array_equal(got.numpy(), want.astype(np.float32))             # integer counts, one division
        assert not got[0].any() and np.all(np.isin(np.round(want.sum(1), 12), (0.0, 1.0)))
    one = torch.full((4, 4), 2, dtype=torch.uint8)
    assert patch_soft_labels(one, 3, 2).tolist() == [[0.0, 0.0, 1.0]] * 4
    with pytest.raises(ValueError, match="label 3 is neither"):
        patch_soft_labels(torch.full((4, 4), 3, dtype=torch.uint8), 3, 2)
    with pytest.raises(ValueError, match="not a multiple of patch"):
        patch_soft_labels(one, 3, 3)
    with pytest.raises(ValueError, match="uint8"):
        patch_soft_labels(one.float(), 3, 2)
    with pytest.raises(ValueError, match="num_classes"):
        patch_soft_labels(one, 1, 2)


def test_context_schedule():
    from dinox.propagate import context_schedule as cs
    assert cs(1, [0], 7) == ({}, [])
    assert cs(2, [0], 7) == ({1: 0}, [(1, [0])])
    assert cs(2, [1], 7) == ({0: 1}, [(0, [1])])
    src, steps = cs(9, [0], 2)                                                  # a seed at the lower end
    assert src == {z: 0 for z in range(1, 9)}
    assert steps == [(1, [0]), (2, [0, 1]), (3, [0, 1, 2]), (4, [0, 2, 3]), (5, [0, 3, 4]), (6, [0, 4, 5]), (7, [0, 5, 6]), (8, [0, 6, 7])]
    src, steps = cs(9, [8], 3)                                                  # ... at the upper end: nearest last
    assert steps[:5] == [(7, [8]), (6, [8, 7]), (5, [8, 7, 6]), (4, [8, 7, 6, 5]), (3, [8, 6, 5, 4])]
    src, steps = cs(9, [2, 6], 7)                                               # two seeds, slice 4 is tied: the lower seed takes it
    assert src == {0: 2, 1: 2, 3: 2, 4: 2, 5: 6, 7: 6, 8: 6}
    assert steps == [(3, [2]), (4, [2, 3]), (1, [2]), (0, [2, 1]), (7, [6]), (8, [6, 7]), (5, [6])]
    src, steps = cs(9, [4], 0)                                                  # no context beside the seed
    assert all(c == [4] for _, c in steps) and [z for z, _ in steps] == [5, 6, 7, 8, 3, 2, 1, 0]
    for Z, seeds, n in ((1, [0], 7), (2, [0], 0), (9, [0], 2), (9, [8], 3), (9, [2, 6], 7), (9, [4], 0), (9, [0, 1, 8], 1), (12, [3, 4, 10], 2)):
        assert cs(Z, seeds, n) == O.context_schedule(Z, seeds, n), (Z, seeds, n)
        src, steps = cs(Z, seeds, n)
        assert sorted(z for z, _ in steps) == sorted(src) == [z for z in range(Z) if z not in seeds]      # every non-seed slice once
    for bad in ((0, [0], 1), (3, [], 1), (3, [3], 1), (3, [0], -1), (3, [True], 1)):
        with pytest.raises(ValueError):
            cs(*bad)


def test_propagate_labels_refuses_bad_input_before_the_device():
    from dinox.propagate import propagate_labels
    lab = torch.zeros((8, 8), dtype=torch.uint8)
    with pytest.raises(ValueError, match="square grid"):
        propagate_labels(torch.zeros(3, 5, 8), {0: lab}, 2, patch=4)
    with pytest.raises(ValueError, match="seeds must be a non-empty dict"):
        propagate_labels(torch.zeros(3, 4, 8), {}, 2, patch=4)
    with pytest.raises(ValueError, match="seed 0 must be uint8"):
        propagate_labels(torch.zeros(3, 4, 8), {0: lab[:4]}, 2, patch=4)
    with pytest.raises(ValueError, match="seeds must be"):
        propagate_labels(torch.zeros(3, 4, 8), {3: lab}, 2, patch=4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        propagate_labels(torch.zeros(3, 4, 8), {0: lab}, 2, patch=4)


# ------------------------------------------------------------------------------------------ script
def test_script_parser(script):
    ap = script.build_parser()
    have = {s for a in ap._actions for s in a.option_strings if s.startswith("--")} - {"--help"}
    assert have == {"--checkpoint", "--volume", "--spacing", "--seed-slice", "--seed-labels", "--num-classes", "--topk", "--context-frames",
                    "--radius", "--temperature", "--amp", "--keep-largest", "--min-component-mm3", "--connectivity", "--out", "--labels",
                    "--report", "--synthetic", "--dump-trace", "--batch-size", "--device"}
    d = ap.parse_args(["--checkpoint", "c.pth", "--num-classes", "3", "--out", "o.npy", "--synthetic", "12"])
    assert (d.topk, d.context_frames, d.radius, d.temperature) == (5, 7, 12, 0.1)      # the DINO protocol's defaults
    assert d.seed_slice is None and not d.amp and not d.keep_largest and d.connectivity == 26 and d.synthetic == 12
    script.check_args(ap, d)
    d = ap.parse_args(["--checkpoint", "c", "--num-classes", "3", "--out", "o.npy", "--volume", "v.npy", "--spacing", "1", "1", "2",
                       "--seed-slice", "3", "--seed-slice", "9", "--seed-labels", "s.npy"])
    assert d.seed_slice == [3, 9] and d.spacing == [1.0, 1.0, 2.0]
    script.check_args(ap, d)
    base = ["--checkpoint", "c", "--num-classes", "3", "--out", "o.npy"]
    for bad in ([], ["--volume", "v.npy"], ["--volume", "v.npy", "--spacing", "1", "1", "1"], ["--volume", "v.npy", "--synthetic", "4"],
                ["--synthetic", "4", "--labels", "g.npy"], ["--synthetic", "4", "--topk", "33"], ["--synthetic", "4", "--temperature", "0"],
                ["--synthetic", "4", "--context-frames", "-1"], ["--volume", "v.npy", "--spacing", "1", "1", "1", "--seed-slice", "2"],
                ["--volume", "v.npy", "--spacing", "1", "1", "1", "--seed-slice", "2", "--seed-labels", "s.npy", "--report", "r.json"]):
        with pytest.raises(SystemExit):
            script.check_args(ap, ap.parse_args(base + bad))
    with pytest.raises(SystemExit):
        script.check_args(ap, ap.parse_args(["--checkpoint", "c", "--num-classes", "1", "--out", "o.npy", "--synthetic", "4"]))
    with pytest.raises(SystemExit, match="computes on MI355X only"):
        script.main(base + ["--synthetic", "4", "--device", "cpu"])


def test_script_synthetic_case_is_deterministic(script):
    vol, lab = script.synthetic_case(12, 56, 3)
    vol2, lab2 = script.synthetic_case(12, 56, 3)
    assert np.array_equal(vol, vol2) and np.array_equal(lab, lab2)
    assert vol.shape == lab.shape == (12, 56, 56) and vol.dtype == np.float32 and lab.dtype == np.uint8
    assert sorted(np.unique(lab)) == [0, 1, 2]
    area = [(lab == c).reshape(12, -1).sum(1) for c in (1, 2)]
    assert all(a[0] > a[-1] > 0 for a in area)                                  # every class in every slice, shrinking along z
    assert all((lab[z] != lab[z + 1]).mean() < 0.05 for z in range(11))         # slowly
    assert script.pick_seed(lab) == 0 and script.pick_seed(lab[::-1]) == 11
    assert vol[lab == 2].mean() > vol[lab == 1].mean() > vol[lab == 0].mean() + 100


# ------------------------------------------------------------------------------------------ oracle self-checks
def test_oracle_identities():
    rng = np.random.default_rng(5)
    g, D, C = 6, 16, 4
    N = g * g
    q = O.unit64(rng.standard_normal((N, D)))
    seg = O.soft_rows(rng, N, C).astype(np.float64)
    out, idx, val = O.propagate_step(q, q, seg, g, 1, 0, 10.0)                  # K = 1, radius 0, context = target: the patch itself
    assert np.array_equal(idx[:, 0], np.arange(N)) and np.array_equal(out, seg)
    k = O.unit64(rng.standard_normal((3 * N, D)))
    S = O.scores64(q, k)
    for radius in (-1, g - 1, g + 5):                                           # a whole-grid radius is an unwindowed top-K
        idx, val = O.select(S, O.window_mask(g, 3, radius), 5)
        order = np.argsort(-S, axis=1, kind="stable")[:, :5]
        assert np.array_equal(idx, order) and np.array_equal(val, np.take_along_axis(S, order, 1))
    for r in (0, 1, 2, 4):                                                      # the clipped window at a corner
        m = O.window_mask(g, 3, r)
        assert m[0].sum() == m[N - 1].sum() == (r + 1) ** 2 * 3
    assert O.window_mask(g, 3, 1)[2 * g + 3].sum() == 9 * 3 and O.window_mask(g, 3, 2)[2 * g + 3].sum() == 25 * 3      # an inner patch
    idx, val = O.select(S, O.window_mask(g, 3, 0), 5)                           # 3 candidates, K = 5: the rest is (-1, -inf)
    assert (idx[:, 3:] == -1).all() and np.isneginf(val[:, 3:]).all() and (idx[:, :3] >= 0).all()
    Sn = S.copy()
    Sn[0] = np.nan                                                              # a NaN query row: nothing enters, the vote is zero
    Sn[:, 7] = np.nan
    idx, val = O.select(Sn, O.window_mask(g, 3, -1), 5)
    assert (idx[0] == -1).all() and not (idx == 7).any()
    assert not O.vote(idx, val, np.ones((3 * N, C)), 10.0)[0].any()
    # ties: equal scores are taken in ascending key order
    idx, _ = O.select(np.zeros((1, 6)), np.array([[True, False, True, True, True, True]]), 3)
    assert idx.tolist() == [[0, 2, 3]]
    # the bound is what its derivation says for a row of equal scores: no argument error, (n + 2) roundings and the exp term of n - 1 weights
    b = O.vote_bound(np.array([[0, 1, 2, -1]]), np.array([[0.5, 0.5, 0.5, -np.inf]]), 10.0)[0]
    assert abs(b - (2 * (O.EXP_REL + O.EXP_FLOOR) + O.gamma(5) + (3 * O.U) ** 2)) < 1e-20
    assert O.vote_bound(np.array([[0, 1]]), np.array([[1.0, -1.0]]), 10.0)[0] <= O.vote_bound_unit(10.0, 2) < 1e-5


# ------------------------------------------------------------------------------------------ input conditions of the GPU float cases
@pytest.mark.parametrize("shape", [s for s in O.SHAPES if s[0] > 1], ids=str)
def test_float_cases_are_mostly_sharp(shape):
    """The GPU float test may only demand index equality on rows whose K-th and (K+1)-th candidate are more than 2 tau apart; the inputs
    are chosen so that this is at least 85 % of the rows, for every K and radius the GPU test runs."""
    g, F, D, C = shape
    q, k, _ = O.float_case(g, F, D, C)
    assert np.allclose(np.linalg.norm(q.astype(np.float64), axis=1), 1.0, atol=1e-6)
    S = O.scores64(q, k)
    tau = 2.0 * D * 2.0 ** -24
    for radius in sorted({O.effective_radius(g, r) for r in O.radii(g)}):
        mask = O.window_mask(g, F, radius)
        for K in O.KS:
            share = O.sharp_rows(S, mask, K, tau).mean()
            assert share >= 0.85, (shape, radius, K, share)


def test_end_to_end_case_is_decided():
    """The float64 propagation of the end-to-end case: at least 99 % of the pixels of the non-seed slices have a top-two class margin
    after bilinear upsampling above twice the vote bound, so the GPU test may demand the hard label there."""
    p = O.E2E
    feats, labs = O.e2e_case()
    Z, g, C, u = p["Z"], p["g"], p["C"], p["patch"]
    unit = O.unit64(feats)
    soft = {p["seed_z"]: O.patch_soft_labels(labs[p["seed_z"]], C, u)}
    _, steps = O.context_schedule(Z, [p["seed_z"]], p["n_context"])
    inv_t = float(np.float32(1.0 / p["temperature"]))
    decided = total = agree = 0
    for z, ctx in steps:
        k = np.concatenate([unit[c] for c in ctx])
        seg = np.concatenate([soft[c] for c in ctx])
        soft[z] = O.propagate_step(unit[z], k, seg, g, p["topk"], p["radius"], inv_t)[0]
        up = np.sort(O.bilinear_upsample(soft[z], g, u), axis=2)
        ok = up[:, :, -1] - up[:, :, -2] > 2 * O.vote_bound_unit(inv_t, p["topk"])
        decided += int(ok.sum())
        total += ok.size
        agree += int((np.argmax(O.bilinear_upsample(soft[z], g, u), 2) == labs[z]).sum())
    assert decided >= 0.99 * total, (decided, total)
    assert agree >= 0.9 * total, (agree, total)                                 # and the case is a meaningful one: the labels do travel
