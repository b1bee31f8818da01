"""GPU checks of the probe block: ``ops.gram`` (csrc/gram.hip) and ``ops.softmax_probe`` (csrc/probe.hip) against float64 NumPy with
bounds derived from the fp32 format, ``dinox.probes`` end to end on the fixture the real reference recorded
(tests/golden/panorgan_probes.npz), and scripts/evaluate_panorgan.py with ``--probes``.  Run with ``-m gpu`` on an MI355X.

Shapes, gram (N, D, ld, column offset): GRAM_SHAPES are the one-tile and small-triangle cases (T = 1 .. 4, element loads but for (513, 64, ld 80)).
GRAM_PATH_SHAPES (tests/test_probes_cpu.py, where a mirror of gram_plan pins each to its path): (300, 1024) T = 8, all 36 tiles and
their inverse map in gram_finish, 16-byte loads, two slabs per split (the prefetch under the products) with a ragged last one;
(700, 768) T = 6; (300, 1023) the same triangle on element loads with a last panel 127 wide; (2000, 384) the statistics shape, off-diagonal
tiles on 16-byte loads, a short last split; (8300, 64) one tile, 260 splits, ragged last slab; (1030, 130, ld 132) 16-byte loads with a quad
across D and a panel two columns wide; (513, 64, ld 80, offset 1) element loads because of the base pointer alone.  The repeated-row
pattern at D = 1024 makes every tile's content a function of its position.
Shapes, softmax_probe (N, D, C, span): PROBE_SHAPES run NB = 1, 2, 3 (D = 384 the only 16-byte-load case) in one trip of the row walk.
PROBE_PATH_SHAPES: D = 385 and 512 run NB = 4 (element / 16-byte loads, 3 / all 32 classes); 513, 768, 1024 run NB = 8 with 3, 2 and 0 idle
column blocks (1024 x 32 classes: the largest LDS and register footprint, also at span 60); N = 16384 is the last size with one row block
per workgroup, 16385 and 16421 send one and two workgroups on a second trip (the last block 1 and 5 rows), (16421, 520) does so on NB = 8.
PROBE_PITCH_SHAPES: D = 66 at pitch 68 is the 16-byte path with a quad across D; D = 64 from column 1 of a pitch-68 buffer is the element
path through the base pointer alone.  (67, 7, 3) carries the non-finite values, in a row that counts and in one that does not."""
import functools
import json
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
from test_probes_cpu import GRAM_PATH_SHAPES, GRAM_PATTERN_SHAPE, PROBE_PATH_SHAPES, PROBE_PITCH_SHAPES

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24                                                 # fp32 unit round-off


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------ gram
GRAM_SHAPES = [(1, 1, 0), (33, 7, 0), (257, 65, 0), (1000, 129, 0), (4099, 385, 0), (513, 64, 80)]      # (N, D, ldx; 0 = D)
GRAM_CASES = ([pytest.param(*s, 0, id="-".join(map(str, s))) for s in GRAM_SHAPES]
              + [pytest.param(*s, id="-".join(map(str, s))) for s in GRAM_PATH_SHAPES])                 # (N, D, ldx, column offset)


def gram_operand(x, ld, off=0):
    """x on the device as columns off .. off + D of the rows of a wider buffer when ld > D (the rest holds NaN: it must never be read
    into a sum).  The buffer is 16-byte aligned, so off = 1 puts the base pointer one float off."""
    if not ld:
        return dev(x)
    buf = torch.full((x.shape[0], ld), float("nan"), device=DEV)
    buf[:, off:off + x.shape[1]] = dev(x)
    return buf[:, off:off + x.shape[1]]


def z64(x, shift):
    z = x if shift is None else (x - shift).astype(np.float32)          # the kernel's z: ONE fp32 subtraction per element
    return z.astype(np.float64)


def run_gram(x, shift, ld, off=0):
    from dinox import ops
    g, cs = ops.gram(gram_operand(x, ld, off), None if shift is None else dev(shift))
    return g.cpu().numpy(), cs.cpu().numpy()


@pytest.mark.parametrize("N,D,ld,off", GRAM_CASES)
def test_gram_integer_rows_are_exact(N, D, ld, off):
    g = np.random.default_rng(N + D)
    x = g.integers(-3, 4, size=(N, D)).astype(np.float32)
    shift = g.integers(-2, 3, size=D).astype(np.float32)
    for s in (None, shift):
        z = z64(x, s)
        G, cs = run_gram(x, s, ld, off)
        assert G.dtype == np.float64 and G.shape == (D, D) and cs.shape == (D,)
        assert np.array_equal(G, z.T @ z) and np.array_equal(cs, z.sum(0))       # |z| <= 5, 25 N < 2^24: every partial sum is an integer below 2^24


def test_gram_repeated_row_pattern_pins_the_tile_maps():
    """x[i, j] = (j % 7) - 3 on every row: gram[a, b] = N z_a z_b, so the content of a 128 x 128 tile is a function of where it lies
    (128 = 2 mod 7) and a tile stored or read at another place shows as a wrong exact integer."""
    N, D = GRAM_PATTERN_SHAPE
    x = np.tile((np.arange(D) % 7 - 3).astype(np.float32), (N, 1))
    shift = (np.arange(D) % 5 - 2).astype(np.float32)
    for s in (None, shift):
        z = z64(x, s)
        G, cs = run_gram(x, s, 0)
        assert np.array_equal(G, N * np.outer(z[0], z[0])) and np.array_equal(cs, N * z[0])        # |z| <= 5, 25 N < 2^24


@pytest.mark.parametrize("N,D,ld,off", GRAM_CASES)
def test_gram_random_rows_within_the_chain_bound(N, D, ld, off):
    g = np.random.default_rng(7 * N + D)
    x = (g.standard_normal((N, D)) + 0.5).astype(np.float32)
    mean = x.astype(np.float64).mean(0).astype(np.float32)
    for s in (None, mean):
        z = z64(x, s)
        G, cs = run_gram(x, s, ld, off)
        err, bound = np.abs(G - z.T @ z), N * U * (np.abs(z).T @ np.abs(z))
        cerr, cbound = np.abs(cs - z.sum(0)), N * U * np.abs(z).sum(0)
        print(f"gram N={N} D={D} ld={ld} off={off} shift={'mean' if s is not None else 'none'}: max err / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}, "
              f"colsum {float((cerr / np.maximum(cbound, 1e-300)).max()):.3f}")
        assert (err <= bound).all() and (cerr <= cbound).all()
        assert np.array_equal(G, G.T)                                            # symmetric to the bit
        G2, cs2 = run_gram(x, s, ld, off)
        assert np.array_equal(G, G2) and np.array_equal(cs, cs2)                 # two launches: the same bits


def test_gram_non_finite_inputs_propagate():
    x = np.random.default_rng(0).standard_normal((300, 70)).astype(np.float32)
    x[17, 3], x[250, 69] = np.inf, np.nan
    G, cs = run_gram(x, None, 0)
    bad = np.zeros(70, bool)
    bad[[3, 69]] = True
    assert not np.isfinite(G[bad]).any() and not np.isfinite(cs[bad]).any() and cs[3] == np.inf
    assert np.isfinite(G[~bad][:, ~bad]).all() and np.isfinite(cs[~bad]).all()


# ------------------------------------------------------------------------------------------ softmax_probe
PROBE_SHAPES = [(1, 1, 2, 8.0), (67, 7, 3, 8.0), (300, 65, 10, 8.0), (1031, 384, 32, 8.0), (2050, 129, 5, 8.0), (300, 65, 10, 60.0)]


@functools.lru_cache(maxsize=None)
def probe_case(N, D, C, span):
    """Operands and the float64 reference (computed once per shape): theta scaled so that the largest |logit| is ``span``."""
    g = np.random.default_rng(1000 * C + D)
    x = g.standard_normal((N, D)).astype(np.float32)
    theta = g.standard_normal((C, D + 1))
    X = np.concatenate([x.astype(np.float64), np.ones((N, 1))], 1)
    theta = (theta * span / np.abs(X @ theta.T).max()).astype(np.float32)
    label = g.integers(0, C, size=N).astype(np.int32)
    return x, label, theta


def probe_reference(x, label, theta):
    N, C = x.shape[0], theta.shape[0]
    X = np.concatenate([x.astype(np.float64), np.ones((N, 1))], 1)
    th = theta.astype(np.float64)
    z = X @ th.T
    m = z.max(1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(z - m).sum(1))
    p = np.exp(z - lse[:, None])
    ok = (label >= 0) & (label < C)
    onehot = np.zeros_like(p)
    onehot[np.nonzero(ok)[0], label[ok]] = 1.0
    loss = float((lse - (z * onehot).sum(1))[ok].sum())
    grad = ((p - onehot) * ok[:, None]).T @ X
    t = (x.shape[1] + 2) * U * float((np.abs(X) @ np.abs(th).T).max())            # bound of a logit's fp32 error
    return p, loss, grad, t, np.abs(X).sum(0)


def run_probe(x, label, theta, ld=0, off=0, **kw):
    from dinox import ops
    loss, grad, prob = ops.softmax_probe(gram_operand(x, ld, off), dev(label), dev(theta), **kw)
    return (None if loss is None else float(loss), None if grad is None else grad.cpu().numpy(), None if prob is None else prob.cpu().numpy())


def check_probe(x, label, theta, what, ld=0, off=0):
    p64, loss64, grad64, t, colabs = probe_reference(x, label, theta)
    loss, grad, prob = run_probe(x, label, theta, ld, off, want_grad=True, want_prob=True)
    N = x.shape[0]
    perr, lerr, gerr = np.abs(prob - p64).max(), abs(loss - loss64), np.abs(grad - grad64)
    gb = (4 * t + 1e-6) * colabs[None, :]
    print(f"softmax_probe {what}: t = {t:.2e}; |p - p64| {perr:.2e} (bound {4 * t + 1e-6:.2e}); |loss - loss64| {lerr:.2e} (bound "
          f"{N * (2 * t + 1e-6):.2e}); err / bound: p {perr / (4 * t + 1e-6):.3f}, loss {lerr / (N * (2 * t + 1e-6)):.3f}, "
          f"grad {float((gerr / gb).max()):.3f}")
    assert np.isfinite(prob).all() and math.isfinite(loss) and np.isfinite(grad).all()
    assert perr <= 4 * t + 1e-6
    assert lerr <= N * (2 * t + 1e-6)
    assert (gerr <= gb).all()
    return loss, grad, prob


def check_probe_three_forms(x, label, theta, what, ld=0, off=0):
    """Full form against float64, then the predict form, a second launch and the gradient-only form: the same bits."""
    loss, grad, prob = check_probe(x, label, theta, what, ld, off)
    _, _, only = run_probe(x, label, theta, ld, off, want_grad=False, want_prob=True)
    assert np.array_equal(only, prob)                                            # predict form: the same bits
    loss2, grad2, prob2 = run_probe(x, label, theta, ld, off, want_grad=True, want_prob=True)
    assert loss2 == loss and np.array_equal(grad2, grad) and np.array_equal(prob2, prob)       # two launches: the same bits
    g_only = run_probe(x, label, theta, ld, off, want_grad=True, want_prob=False)
    assert g_only[2] is None and g_only[0] == loss and np.array_equal(g_only[1], grad)
    return loss, grad, prob


@pytest.mark.parametrize("N,D,C,span", PROBE_SHAPES + PROBE_PATH_SHAPES)
def test_softmax_probe_against_float64(N, D, C, span):
    x, label, theta = probe_case(N, D, C, span)
    check_probe_three_forms(x, label, theta, f"N={N} D={D} C={C} span={span}")


@pytest.mark.parametrize("N,D,C,ld,off", PROBE_PITCH_SHAPES)
def test_softmax_probe_row_loads_at_a_whole_quad_pitch(N, D, C, ld, off):
    """Rows of a NaN-filled buffer whose pitch is a multiple of four floats: 16-byte loads with the last quad across D when the base is
    aligned, element loads when only the base pointer is off.  A load past D would bring a NaN into the image."""
    x, label, theta = probe_case(N, D, C, 8.0)
    loss, grad, prob = check_probe_three_forms(x, label, theta, f"N={N} D={D} C={C} ld={ld} off={off}", ld, off)
    plain = run_probe(x, label, theta, want_grad=True, want_prob=True)           # the same rows, contiguous: the same arithmetic
    assert plain[0] == loss and np.array_equal(plain[1], grad) and np.array_equal(plain[2], prob)


@pytest.mark.parametrize("N,D,C,span", [(16421, 7, 3, 8.0), (16421, 520, 4, 8.0)])
def test_softmax_probe_second_trip_of_rows_that_do_not_count(N, D, C, span):
    """Every row of the second trip (rows 16384 .. 16420, two workgroups) has a label out of range.  Loss and gradient are those of the
    float64 reference without these rows; their probabilities are still written; and, since such a row adds exact zeros to what a
    workgroup carries, the sums have the bits of a call on the first 16384 rows alone.  (At D = 520 the a-priori bound of the intercept
    gradient, (4 t + 1e-6) N, is wider than what one lost block of 32 rows can change: there the equality of bits is the check of the
    carried sums, on NB = 8.)"""
    assert (N, D, C, span) in PROBE_PATH_SHAPES                                  # pinned to blocks = 514 > groups = 512 by the CPU test
    x, label, theta = probe_case(N, D, C, span)
    label = label.copy()
    label[16384:] = np.resize(np.array([-1, C, 2 ** 30, -7, -2 ** 31], np.int64), N - 16384).astype(np.int32)
    loss, grad, prob = check_probe(x, label, theta, f"N={N} D={D} C={C}, second trip dropped")       # the reference leaves those rows out
    head = run_probe(x[:16384], label[:16384], theta, want_grad=True, want_prob=True)
    assert head[0] == loss and np.array_equal(head[1], grad) and np.array_equal(head[2], prob[:16384])


@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")], ids=["nan", "inf", "-inf"])
def test_softmax_probe_non_finite_value_in_a_row_that_counts(value):
    """A NaN or infinite logit in a counting row: the row's probabilities and the loss are non-finite (the row does not vanish), every
    other row's probabilities keep their bits (rows are independent columns of the logit product), and the call returns."""
    x, label, theta = probe_case(67, 7, 3, 8.0)
    assert (theta[:, 2] != 0).all()
    _, _, clean = run_probe(x, label, theta, want_grad=True, want_prob=True)
    x = x.copy()
    x[40, 2] = value
    loss, grad, prob = run_probe(x, label, theta, want_grad=True, want_prob=True)
    keep = np.arange(67) != 40
    assert not np.isfinite(prob[40]).all() and not math.isfinite(loss)
    assert np.isfinite(clean).all() and np.array_equal(prob[keep], clean[keep])
    _, _, only = run_probe(x, label, theta, want_grad=False, want_prob=True)
    assert np.array_equal(only, prob, equal_nan=True)                            # predict form: the same bits


def test_softmax_probe_rows_of_a_wider_buffer():
    """ldx > D, rows not 16-byte aligned: the element-load path; the padding holds NaN and must never be read."""
    x, label, theta = probe_case(300, 65, 10, 8.0)
    from dinox import ops
    buf = torch.full((300, 71), float("nan"), device=DEV)
    buf[:, 3:68] = dev(x)
    loss, grad, prob = ops.softmax_probe(buf[:, 3:68], dev(label), dev(theta), want_grad=True, want_prob=True)
    want = run_probe(x, label, theta, want_grad=True, want_prob=True)
    p64, loss64, grad64, t, colabs = probe_reference(x, label, theta)
    assert np.abs(prob.cpu().numpy() - p64).max() <= 4 * t + 1e-6 and abs(float(loss) - loss64) <= 300 * (2 * t + 1e-6)
    assert (np.abs(grad.cpu().numpy() - grad64) <= (4 * t + 1e-6) * colabs[None, :]).all()
    assert np.isfinite(want[2]).all()


def test_softmax_probe_out_of_range_labels_contribute_nothing():
    from dinox import ops
    x, label, theta = probe_case(2050, 129, 5, 8.0)
    wild = label.astype(np.int64)
    wild[[0, 31, 32, 700, 2049]] = [-1, 5, 2 ** 30, 2 ** 32 + 1, -2 ** 31]       # (int64 labels must not wrap into range either)
    ok = (wild >= 0) & (wild < 5)
    loss, grad, prob = ops.softmax_probe(dev(x), dev(wild), dev(theta), want_grad=True, want_prob=True)
    as32 = np.where(ok, wild, np.array([-1, 5, 2 ** 30, -7, -2 ** 31] * 410)[:2050]).astype(np.int32)
    loss32, grad32, prob32 = run_probe(x, as32, theta, want_grad=True, want_prob=True)
    assert float(loss) == loss32 and np.array_equal(grad.cpu().numpy(), grad32) and np.array_equal(prob.cpu().numpy(), prob32)
    p64, loss64, grad64, t, colabs = probe_reference(x, as32, theta)          # the reference leaves those rows out
    assert abs(loss32 - loss64) <= 2050 * (2 * t + 1e-6) and (np.abs(grad32 - grad64) <= (4 * t + 1e-6) * colabs[None, :]).all()
    assert np.abs(prob32 - p64).max() <= 4 * t + 1e-6                            # their probabilities are still written
    # the same rows removed give the same sums up to the bound (other workgroup boundaries: not the same bits)
    lossk, gradk, _ = run_probe(x[ok], as32[ok], theta, want_grad=True, want_prob=True)
    assert abs(lossk - loss32) <= 2 * 2050 * (2 * t + 1e-6) and (np.abs(gradk - grad32) <= 2 * (4 * t + 1e-6) * colabs[None, :]).all()


def test_softmax_probe_gradient_is_the_derivative_of_the_loss():
    """Central difference of the kernel's loss along a random direction against grad . d.  The truncation error is measured on the float64
    function itself; the two losses carry at most N (2 t + 1e-6) each."""
    x, label, theta = probe_case(67, 7, 3, 8.0)
    d = np.random.default_rng(5).standard_normal(theta.shape)
    d /= np.abs(d).sum()
    h = 2.0 ** -6
    up, dn = (theta + h * d).astype(np.float32), (theta - h * d).astype(np.float32)
    step = (up.astype(np.float64) - dn.astype(np.float64))                       # the step actually taken, after rounding to fp32
    _, grad, _ = run_probe(x, label, theta, want_grad=True)
    lu, ld_ = run_probe(x, label, up, want_grad=True)[0], run_probe(x, label, dn, want_grad=True)[0]
    _, lu64, _, tu, _ = probe_reference(x, label, up)
    _, ld64, g64, t, colabs = probe_reference(x, label, theta)
    ld64 = probe_reference(x, label, dn)[1]
    truncation = abs((lu64 - ld64) - float((g64 * step).sum()))
    noise = 2 * 67 * (2 * tu + 1e-6) + float(((4 * t + 1e-6) * colabs[None, :] * np.abs(step)).sum())
    got = abs((lu - ld_) - float((grad * step).sum()))
    print(f"finite difference: |dL - g.step| = {got:.3e}, truncation {truncation:.3e}, noise bound {noise:.3e}, dL = {lu - ld_:.6f}")
    assert got <= truncation + noise and abs(lu - ld_) > 20 * (truncation + noise)       # the check has teeth: the signal is far above its slack


# ------------------------------------------------------------------------------------------ end to end on the reference's fixture
TAU_P_FIXED = 1e-3           # the fixture's margins (0.02 top-2 gap, 2e-3 pair window) are built for a fit within 1e-3 of the optimum
TAU_P = 7.5e-4               # 10 x the distance measured on MI355X, 7.43e-5 ("Probes")


@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(os.path.join(GOLDEN, "panorgan_probes.npz"))
    names = [str(s) for s in z["label_names"]]
    ref = {k: json.loads(str(z[f"reference_{k}"])) for k in ("probe", "ridge", "stats")}
    return z, dev(z["rows"]), [names[i] for i in z["labels"]], [str(s) for s in z["series"]], z["spacings"], ref


def test_logistic_probe_on_the_fixture():
    from dinox import probes
    z, E, labels, series, _, ref = fixture()
    want = ref["probe"]
    got = probes.logistic_probe(E, labels, series, seed=42, return_details=True)
    prob, fit = got.pop("probabilities"), got.pop("fit")
    tau = float(np.abs(prob - z["prob_tight"]).max())
    print(f"logistic_probe: fit {fit}; tau_p = max |p - prob_tight| = {tau:.3e} (reference's own default fit: {float(z['prob_default_distance']):.3e}); "
          f"auc {got['auc']:.9f}, tight {float(z['auc_tight']):.9f}, reference {want['auc']:.9f}")
    assert list(got) == list(want)
    for key in ("labels", "train_series", "test_series", "train_slices", "test_slices", "note", "accuracy", "accuracy_ci95"):
        assert got[key] == want[key], key
    slack = float(z["auc_slack"])
    assert abs(got["auc"] - float(z["auc_tight"])) <= slack + 1e-12
    assert abs(got["auc"] - want["auc"]) <= slack + abs(want["auc"] - float(z["auc_tight"])) + 1e-12
    assert TAU_P <= TAU_P_FIXED and tau <= TAU_P
    assert fit["evaluations"] <= 2000


def test_spacing_ridge_on_the_fixture():
    from dinox import probes
    _, E, labels, series, spacings, ref = fixture()
    want = ref["ridge"]
    got = probes.spacing_ridge(E, spacings, labels, series, seed=42)
    print(f"spacing_ridge: r2 {got['r2']:.9f} vs {want['r2']:.9f}, mae {got['mae_log_spacing']:.9f} vs {want['mae_log_spacing']:.9f}")
    assert list(got) == list(want) and all(got[k] == want[k] for k in ("target", "train_slices", "test_slices", "note"))
    assert abs(got["r2"] - want["r2"]) <= 1e-5 and abs(got["mae_log_spacing"] - want["mae_log_spacing"]) <= 1e-5


def test_embedding_stats_on_the_fixture():
    from dinox import probes
    _, E, labels, _, spacings, ref = fixture()
    want = ref["stats"]
    got = probes.embedding_stats(E, spacings, labels)
    assert list(got["per_dataset"]) == list(want["per_dataset"])
    for name, w in want["per_dataset"].items():
        g = got["per_dataset"][name]
        print(f"embedding_stats {name}: " + ", ".join(f"{k} {g[k]:.9f} vs {w[k]:.9f}" for k in list(w)[1:]))
        assert list(g) == list(w) and g["n"] == w["n"]
        assert abs(g["embedding_std"] - w["embedding_std"]) <= 1e-6 and abs(g["intra_cosine_to_centroid"] - w["intra_cosine_to_centroid"]) <= 1e-6
        assert abs(abs(g["pca1_spacing_correlation"]) - abs(w["pca1_spacing_correlation"])) <= 1e-5
    assert list(got["cross_dataset_centroid_cosine"]) == list(want["cross_dataset_centroid_cosine"])
    for pair, w in want["cross_dataset_centroid_cosine"].items():
        assert abs(got["cross_dataset_centroid_cosine"][pair] - w) <= 1e-6


# ------------------------------------------------------------------------------------------ script
def finite_or_error(v, path=""):
    if isinstance(v, dict):
        if set(v) == {"error"}:
            return
        for k, w in v.items():
            finite_or_error(w, f"{path}/{k}")
    elif isinstance(v, list):
        for i, w in enumerate(v):
            finite_or_error(w, f"{path}[{i}]")
    elif isinstance(v, float):
        assert math.isfinite(v), path


def test_script_with_and_without_probes(tmp_path):
    ckpt = tmp_path / "ref_checkpoint_00000003.pth"
    shutil.copy(os.path.join(GOLDEN, "ref_checkpoint_00000003.pth"), ckpt)
    script = os.path.join(ROOT, "dino-x_amd", "scripts", "evaluate_panorgan.py")
    runs = {}
    for flag in ("--probes", "--skip-probes"):
        out = tmp_path / f"eval{flag}.json"
        p = subprocess.run([sys.executable, script, "--checkpoint", str(ckpt), "--synthetic", "512", "--scale-aware", "--out", str(out), flag],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        print(p.stdout)
        print(p.stderr[-2000:])
        assert p.returncode == 0, p.stderr[-2000:]
        assert p.stdout.splitlines()[-1] == "ok=true"
        runs[flag] = (json.loads(out.read_text()), p.stdout.splitlines())
    m, lines = runs["--probes"]
    assert list(m["metrics"]) == ["domain_clustering", "knn_probe", "dataset_discrimination_probe", "spacing_prediction", "embedding_stats"]
    finite_or_error(m["metrics"])
    probe, ridge, stats = (m["metrics"][k] for k in ("dataset_discrimination_probe", "spacing_prediction", "embedding_stats"))
    assert probe["labels"] == m["datasets"] and probe["train_slices"] + probe["test_slices"] == 512 and 0.0 <= probe["accuracy"] <= 1.0
    assert probe["train_series"] + probe["test_series"] == 24                    # 8 synthetic series x 3 datasets: a series has one dataset
    assert ridge["train_slices"] == probe["train_slices"] and list(stats["per_dataset"]) == m["datasets"]
    assert sum(d["n"] for d in stats["per_dataset"].values()) == 512 and len(stats["cross_dataset_centroid_cosine"]) == 3
    assert f"  Accuracy: {probe['accuracy']:.3f} (CI: {probe['accuracy_ci95']})" in lines and f"  AUC: {probe['auc']:.3f}" in lines
    assert f"  R²: {ridge['r2']:.3f}" in lines and f"  MAE(log spacing): {ridge['mae_log_spacing']:.4f}" in lines
    assert sum(line.startswith("  Cross: ") for line in lines) == 3
    # without the probes: the file of a run that never heard of them
    plain, plain_lines = runs["--skip-probes"]
    assert list(plain["metrics"]) == ["domain_clustering", "knn_probe"]
    for key in plain:
        if key not in ("created_at", "seconds", "metrics"):
            assert plain[key] == m[key], key
    assert plain["metrics"] == {k: m["metrics"][k] for k in ("domain_clustering", "knn_probe")}
    assert not any("[3/5]" in line or "Cross:" in line for line in plain_lines)


def test_softmax_probe_row_that_does_not_count_cannot_poison_the_gradient():
    """A non-finite value in a row whose label is out of range: its probabilities are non-finite, loss and gradient are those of the
    other rows (the row is taken out of the image before R^T X: 0 * inf would be NaN)."""
    x, label, theta = probe_case(67, 7, 3, 8.0)
    x, label = x.copy(), label.copy()
    x[40, 2], label[40] = np.inf, -1
    loss, grad, prob = run_probe(x, label, theta, want_grad=True, want_prob=True)
    keep = np.arange(67) != 40
    p64, loss64, grad64, t, colabs = probe_reference(x[keep], label[keep], theta)
    assert not np.isfinite(prob[40]).all() and np.isfinite(prob[keep]).all()
    assert abs(loss - loss64) <= 67 * (2 * t + 1e-6) and (np.abs(grad - grad64) <= (4 * t + 1e-6) * colabs[None, :]).all()
