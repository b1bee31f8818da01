"""GPU checks of dense label propagation (csrc/labelprop.hip, dinox/propagate.py, scripts/propagate_volume.py) against the float64 oracle
of tests/_labelprop_oracle.py, whose docstring derives the bound of the vote used here.  Shapes are the smallest at which each path can
break: N = 196 is one full and one partial strip, (5, 8, 7, 3) is less than a tile with a non-vector D, (28, 8, 384, 4) has 49 key
tiles, key splits and skipped tiles, (1, 1, 1, 2) is one patch, (9, 2, 88, 64) the widest vote."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _labelprop_oracle as O
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = 0.1
INV_T = float(np.float32(1.0 / T))


def run(q, k, seg, g, K, radius, temperature=T):
    from dinox import ops
    out, idx, val = ops.label_propagate(torch.as_tensor(q).to(DEV), torch.as_tensor(k).to(DEV), torch.as_tensor(seg).to(DEV), g, K=K,
                                        radius=radius, temperature=temperature)
    return out.cpu().numpy(), idx.cpu().numpy(), val.cpu().numpy()


def check_vote(out, idx, val, seg, what):
    """out against the float64 vote on the kernel's own (idx, val), within the derived bound."""
    want = O.vote(idx, val, seg, INV_T)
    bound = O.vote_bound(idx, val, INV_T)
    err = np.abs(out.astype(np.float64) - want).max(1)
    worst = int(np.argmax(err - bound))
    print(f"{what}: max vote error {err.max():.3e}, bound there {bound[np.argmax(err)]:.3e}")
    assert (err <= bound).all(), (what, worst, err[worst], bound[worst])


_selected = {}


def selected(kind, shape, radius):
    """The oracle's K = 32 selection (shorter K are its prefixes), computed once per case and effective radius."""
    g, F, D, C = shape
    key = (kind, shape, O.effective_radius(g, radius))
    if key not in _selected:
        q, k, _ = (O.exact_case if kind == "exact" else O.float_case)(*shape)
        _selected[key] = O.select(O.scores64(q, k), O.window_mask(g, F, radius), 32)
    return _selected[key]


# ------------------------------------------------------------------------------------------ 1. exact
@pytest.mark.parametrize("shape", O.SHAPES, ids=str)
def test_exact_selection_and_vote(shape):
    g, F, D, C = shape
    q, k, seg = O.exact_case(*shape)
    for radius in O.radii(g):
        widx, wval = selected("exact", shape, radius)
        for K in O.KS:
            out, idx, val = run(q, k, seg, g, K, radius)
            assert np.array_equal(idx, widx[:, :K]), (shape, K, radius)
            assert np.array_equal(val, wval[:, :K].astype(np.float32)), (shape, K, radius)      # integers (and -inf): exact
            check_vote(out, idx, val, seg, f"exact {shape} K={K} r={radius}")
    out, idx, val = run(q, k, seg, g, 5, 0)                                     # radius 0: F candidates, the rest is (-1, -inf)
    n = min(F, 5)
    assert (idx[:, :n] >= 0).all() and (idx[:, n:] == -1).all() and np.isneginf(val[:, n:]).all() and np.isfinite(val[:, :n]).all()


# ------------------------------------------------------------------------------------------ 2. knn_topk
@pytest.mark.parametrize("shape", O.SHAPES, ids=str)
def test_whole_grid_is_bitwise_knn_topk(shape):
    from dinox import ops
    g, F, D, C = shape
    for kind in (O.exact_case, O.float_case):
        q, k, seg = (torch.from_numpy(a).to(DEV) for a in kind(*shape))
        for K in O.KS:
            kidx, kval = ops.knn_topk(q, k, K)
            for radius in (-1, g - 1, g + 5):
                _, idx, val = ops.label_propagate(q, k, seg, g, K=K, radius=radius)
                assert torch.equal(idx, kidx) and torch.equal(val.view(torch.int32), kval.view(torch.int32)), (shape, K, radius)


# ------------------------------------------------------------------------------------------ 3. float
@pytest.mark.parametrize("shape", O.SHAPES, ids=str)
def test_float_selection_and_vote(shape):
    g, F, D, C = shape
    q, k, seg = O.float_case(*shape)
    S = O.scores64(q, k)
    eps = D * 2.0 ** -24
    tau = 2 * eps
    for radius in O.radii(g):
        mask = O.window_mask(g, F, radius)
        Sm = np.where(mask, S, -np.inf)
        widx, _ = selected("float", shape, radius)
        for K in O.KS:
            out, idx, val = run(q, k, seg, g, K, radius)
            what = (shape, K, radius)
            filled = idx >= 0
            safe = np.where(filled, idx, 0)
            assert (np.take_along_axis(mask, safe, 1) | ~filled).all(), what                    # never a key from outside the window
            assert np.array_equal(filled.sum(1), np.minimum(mask.sum(1), K)), what
            s64 = np.take_along_axis(S, safe, 1)
            assert (np.abs(val - s64)[filled] <= eps).all(), what
            with np.errstate(invalid="ignore"):                                                 # (-inf - -inf between two empty slots)
                step = np.diff(val.astype(np.float64), axis=1)
            assert (step[filled[:, 1:]] <= 0).all(), what                                       # order violations: none
            same_score = (step == 0) & filled[:, 1:]
            assert (np.diff(idx, axis=1)[same_score] > 0).all(), what
            for p in range(g * g):
                assert len(set(idx[p][filled[p]])) == filled[p].sum(), what
            sK = -np.sort(-Sm, axis=1)[:, min(K, Sm.shape[1]) - 1]                               # the K-th float64 candidate score
            full = np.isfinite(sK)
            assert (s64[full] >= sK[full, None] - tau).all(), what                              # no chosen key below s_K - tau
            must = Sm > sK[:, None] + tau                                                       # no candidate above s_K + tau missed
            chosen = np.zeros_like(mask)
            chosen[np.nonzero(filled)[0], idx[filled]] = True
            assert not (must & ~chosen).any(), what
            sharp = O.sharp_rows(S, mask, K, tau)
            assert sharp.mean() >= 0.85, what
            assert np.array_equal(np.sort(idx[sharp], 1), np.sort(widx[sharp, :K], 1)), what    # sharp rows: the oracle's set
            check_vote(out, idx, val, seg, f"float {what}")


# ------------------------------------------------------------------------------------------ 4. identities
def test_identities_and_non_finite_rows():
    g, F, D, C = 14, 1, 32, 5
    q, _, seg = O.float_case(g, F, D, C)
    out, idx, val = run(q, q, seg, g, 1, 0)                                     # K = 1, radius 0, context = target
    assert np.array_equal(idx[:, 0], np.arange(g * g)) and np.array_equal(out.view(np.int32), seg.view(np.int32))
    q, k, seg = O.float_case(14, 3, 32, 5)
    seg2 = seg.copy()
    seg2[::2] = 0.0                                                             # zero rows vote zero and nothing is renormalised
    out, idx, val = run(q, k, seg2, 14, 5, 3)
    check_vote(out, idx, val, seg2, "zero seg rows")
    assert (out.sum(1) < 0.999).any() and not run(q, k, np.zeros_like(seg), 14, 5, 3)[0].any()
    qn, kn = q.copy(), k.copy()
    qn[7] = np.nan
    kn[40, 3] = np.nan
    kn[250] = np.nan
    out, idx, val = run(qn, kn, seg, 14, 5, -1)
    assert (idx[7] == -1).all() and np.isneginf(val[7]).all() and not out[7].any()
    assert not np.isin(idx, (40, 250)).any() and np.isfinite(out).all()
    rest = np.arange(196) != 7
    assert (idx[rest] >= 0).all()
    check_vote(out[rest], idx[rest], val[rest], seg, "NaN keys")


# ------------------------------------------------------------------------------------------ 5. determinism, strided views
def test_two_runs_are_bit_identical_and_strided_views_equal_copies():
    from dinox import ops
    for shape in ((28, 8, 384, 4), (5, 8, 7, 3)):
        g, F, D, C = shape
        q, k, seg = (torch.from_numpy(a).to(DEV) for a in O.float_case(*shape))
        a = ops.label_propagate(q, k, seg, g, K=5, radius=3)
        b = ops.label_propagate(q, k, seg, g, K=5, radius=3)
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))
        for pad in (4, 1):                                                      # a leading dimension that keeps / breaks 16-byte rows
            qw = torch.full((g * g, D + pad), float("nan"), device=DEV)
            kw = torch.full((F * g * g, D + pad), float("nan"), device=DEV)
            qw[:, :D], kw[:, :D] = q, k
            c = ops.label_propagate(qw[:, :D], kw[:, :D], seg, g, K=5, radius=3)
            assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, c)), (shape, pad)
        c = ops.label_propagate(q.t().contiguous().t(), k, seg, g, K=5, radius=3)      # column-major: copied
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, c))


# ------------------------------------------------------------------------------------------ 6. slot order
def test_permuting_the_context_slots():
    g, F, D, C = 14, 3, 32, 5
    N = g * g
    q, k, seg = O.float_case(g, F, D, C)
    perm = [2, 0, 1]                                                            # new slot f holds old slot perm[f]
    kp = np.concatenate([k[f * N:(f + 1) * N] for f in perm])
    sp = np.concatenate([seg[f * N:(f + 1) * N] for f in perm])
    for K, radius in ((5, 3), (32, 1), (1, -1)):
        out, idx, val = run(q, k, seg, g, K, radius)
        outp, idxp, valp = run(q, kp, sp, g, K, radius)
        assert np.array_equal(val.view(np.int32), valp.view(np.int32))
        back = np.where(idxp >= 0, np.array(perm)[np.maximum(idxp, 0) // N] * N + np.maximum(idxp, 0) % N, -1)      # in the old numbering
        # equal scores are ordered by index, which the permutation changes: compare as sets, row by row, between ties
        untied = np.ones(N, bool)
        for p in range(N):
            if sorted(back[p]) != sorted(idx[p]):
                untied[p] = False
        S = O.scores64(q, k)
        Sm = np.where(O.window_mask(g, F, radius), S, -np.inf)
        top = -np.sort(-Sm, axis=1)
        cut = (top[:, K - 1] == top[:, K]) if top.shape[1] > K else np.zeros(N, bool)          # a tie at the K-th score cuts the set
        assert (untied | cut).all()
        rows = ~cut
        want = O.vote(idx, val, seg, INV_T)
        assert (np.abs(outp[rows].astype(np.float64) - want[rows]).max(1) <= O.vote_bound(idx, val, INV_T)[rows]).all()


# ------------------------------------------------------------------------------------------ 7. propagate_labels end to end
def test_propagate_labels_end_to_end_teacher_forced():
    from dinox import ops
    from dinox.propagate import propagate_labels
    p = O.E2E
    Z, g, C, u, sz = p["Z"], p["g"], p["C"], p["patch"], p["seed_z"]
    N, S = g * g, g * u
    feats, labs = O.e2e_case()
    f = torch.from_numpy(feats).to(DEV)
    seeds = {sz: torch.from_numpy(labs[sz]).to(DEV)}
    soft, hard, trace = propagate_labels(f, seeds, C, patch=u, n_context=p["n_context"], topk=p["topk"], radius=p["radius"],
                                         temperature=p["temperature"], return_trace=True)
    assert tuple(soft.shape) == (Z, N, C) and soft.is_cuda and hard.dtype == torch.uint8 and tuple(hard.shape) == (Z, S, S)
    unit = ops.normalize_rows(f.reshape(Z * N, -1))[0].view(Z, N, -1).cpu().numpy()      # the fp32 rows the kernel multiplied
    soft_h, hard_h = soft.cpu().numpy(), hard.cpu().numpy()
    assert np.array_equal(hard_h[sz], labs[sz])                                 # the seed returns its own map
    assert np.array_equal(soft_h[sz], O.patch_soft_labels(labs[sz], C, u).astype(np.float32))
    source, steps = O.context_schedule(Z, [sz], p["n_context"])
    assert [(t["z"], sorted(t["slots"])) for t in trace] == [(z, sorted(c)) for z, c in steps] and all(t["slots"][0] == sz for t in trace)
    inv_t = float(np.float32(1.0 / p["temperature"]))
    eps = feats.shape[2] * 2.0 ** -24
    tau = 2 * eps
    bound2 = 2 * O.vote_bound_unit(inv_t, p["topk"])
    decided = total = undecided_wrong = 0
    for t in trace:
        z = t["z"]
        k = np.concatenate([unit[c] for c in t["slots"]])                       # this step's own recorded context
        seg = np.concatenate([soft_h[c] for c in t["slots"]])
        idx, val, out = (t[n].cpu().numpy() for n in ("idx", "val", "out"))
        assert np.array_equal(out, soft_h[z])
        S64 = O.scores64(unit[z], k)
        mask = O.window_mask(g, len(t["slots"]), p["radius"])
        widx, wval = O.select(S64, mask, p["topk"])
        assert (np.abs(val - np.take_along_axis(S64, idx, 1)) <= eps).all() and np.take_along_axis(mask, idx, 1).all()
        sharp = O.sharp_rows(S64, mask, p["topk"], tau)
        assert np.array_equal(np.sort(idx[sharp], 1), np.sort(widx[sharp], 1))
        want = O.vote(idx, val, seg, inv_t)
        assert (np.abs(out.astype(np.float64) - want).max(1) <= O.vote_bound(idx, val, inv_t)).all(), z
        up = O.bilinear_upsample(want, g, u)
        top = np.sort(up, axis=2)
        ok = top[:, :, -1] - top[:, :, -2] > bound2
        assert np.array_equal(hard_h[z][ok], np.argmax(up, 2)[ok].astype(np.uint8)), z
        decided += int(ok.sum())
        total += ok.size
        undecided_wrong += int((hard_h[z][~ok] != np.argmax(up, 2)[~ok]).sum())
    print(f"decided pixels {decided} of {total}; undecided {total - decided}, of which {undecided_wrong} differ from the float64 argmax")
    assert decided >= 0.99 * total


def test_propagate_labels_identical_planes_and_two_seed_tie():
    from dinox.propagate import propagate_labels
    p = O.E2E
    Z, C, u = p["Z"], p["C"], p["patch"]
    feats, labs = O.e2e_case("same")
    f = torch.from_numpy(feats).to(DEV)
    lab0 = torch.from_numpy(labs[0]).to(DEV)
    soft, hard = propagate_labels(f, {3: lab0}, C, patch=u, n_context=2, topk=1, radius=0)
    assert all(torch.equal(hard[z], lab0) for z in range(Z))                    # every patch finds itself: the seed's map on every slice
    assert all(torch.equal(soft[z].view(torch.int32), soft[3].view(torch.int32)) for z in range(Z))
    # two seeds with different maps on identical planes: every slice takes its source seed's map, slice 4 (tied) the lower seed's
    other = torch.from_numpy(np.ascontiguousarray(labs[0].T)).to(DEV)
    soft, hard, trace = propagate_labels(f, {2: lab0, 6: other}, C, patch=u, n_context=2, topk=1, radius=0, return_trace=True)
    assert {t["z"]: t["seed"] for t in trace} == {0: 2, 1: 2, 3: 2, 4: 2, 5: 6, 7: 6, 8: 6}
    for z in range(Z):
        assert torch.equal(hard[z], lab0 if z <= 4 else other), z


# ------------------------------------------------------------------------------------------ 8. script
def test_script_on_a_synthetic_series(tmp_path):
    from dinox import ops
    script = os.path.join(ROOT, "dino-x_amd", "scripts", "propagate_volume.py")
    ckpt = os.path.join(GOLDEN, "ref_checkpoint_00000003.pth")
    C = 3

    def go(name, *extra):
        out, rep, tr = tmp_path / f"{name}.npy", tmp_path / f"{name}.json", tmp_path / f"{name}.npz"
        r = subprocess.run([sys.executable, script, "--checkpoint", ckpt, "--synthetic", "12", "--num-classes", str(C), "--out", str(out),
                            "--report", str(rep), "--dump-trace", str(tr), *extra], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        text = r.stdout.decode()
        assert r.returncode == 0, text
        assert text.strip().splitlines()[-1] == "ok=true", text
        return np.load(out), json.loads(rep.read_text()), np.load(tr)

    labels, report, trace = go("plain")
    import importlib.util
    mspec = importlib.util.spec_from_file_location("propagate_volume", script)
    mod = importlib.util.module_from_spec(mspec)
    mspec.loader.exec_module(mod)                                               # the script's own synthetic case and report keys
    spec = vars(mod)
    assert tuple(report) == spec["REPORT_KEYS"]
    Z, S = labels.shape[0], labels.shape[1]
    _, gt = spec["synthetic_case"](12, S, C)
    assert labels.dtype == np.uint8 and labels.shape == gt.shape
    seed = spec["pick_seed"](gt)
    assert report["seeds"] == [seed] and report["slices"] == Z == 12 and np.array_equal(labels[seed], gt[seed])
    assert report["params"]["topk"] == 5 and report["params"]["context_frames"] == 7 and report["params"]["radius"] == 12

    def dice(sel):
        return [2.0 * ((labels[sel] == c) & (gt[sel] == c)).sum() / max(((labels[sel] == c).sum() + (gt[sel] == c).sum()), 1) for c in range(C)]

    rest = [z for z in range(Z) if z != seed]
    assert np.allclose(report["per_class"]["dice"], dice(rest), atol=1e-12)
    assert abs(report["mean"]["dice"] - np.mean(dice(rest)[1:])) <= 1e-12
    bins = report["by_distance"]
    assert sorted(int(d) for d in bins) == sorted({abs(z - seed) for z in rest}) and sum(b["slices"] for b in bins.values()) == len(rest)
    for d, b in bins.items():
        assert np.allclose(b["dice"], dice([z for z in rest if abs(z - seed) == int(d)]), atol=1e-12)
    assert sorted(trace["z"].tolist()) == rest and (trace["slots"][:, 0] == seed).all() and trace["idx"].shape[0] == len(rest)

    labels, report, _ = go("largest", "--keep-largest")
    assert report["params"]["keep_largest"] is True
    _, _, ncomp = ops.cc_label_3d(torch.from_numpy(labels).to(DEV), C)
    assert (ncomp[1:] <= 1).all(), ncomp
    assert np.allclose(report["per_class"]["dice"], dice(rest), atol=1e-12)
