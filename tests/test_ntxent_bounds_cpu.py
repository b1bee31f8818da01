"""The elementwise NT-Xent bounds of oracle/ntxent_bounds.py, proved without a GPU:

  * the float64 statements agree with tests/_ntxent_oracle.py and tests/_ntxent_dp_oracle.py on a symmetric S, and give the known
    answers of a collapsed batch and of M = 2;
  * the fp32 emulation of the kernels' own order stays inside every bound on every (family, shape, tau) that
    tests/test_ntxent_bounds_gpu.py launches (the largest ratio per output is printed);
  * every planted defect (NB.MUTANTS) leaves a bound, or a canary, on at least one of those cases.
"""
import math

import numpy as np
import pytest

import _ntxent_dp_oracle as DPO
import _ntxent_oracle as NX
import _small_kernels_oracle as SO
from oracle import ntxent_bounds as NB

F32, F64 = np.float32, np.float64
WORST = {}


def note(kernel, ratio):
    WORST[kernel] = max(WORST.get(kernel, 0.0), ratio)
    return ratio


def test_the_expf_logf_allowance_is_the_projects_own():
    assert NB.EXP_LOG_RTOL == SO.CE_LOSS_RTOL


# ------------------------------------------------------------------------------------------ the statements
@pytest.mark.parametrize("M,tau", [(6, 0.1), (66, 0.07), (258, 0.5)])
def test_statements_agree_with_the_square_oracle(M, tau):
    """On the exactly symmetric float64 S of unit rows: lse, loss and W zh as _ntxent_oracle.ntxent has them."""
    z = NB.make_z("randn", M).astype(F32)
    zh, n = NX.normalize(z)
    S = zh @ zh.T
    it = NB.f32(1.0 / tau)
    r = NB.rows_ref(np.where(np.eye(M, dtype=bool), np.nan, S), it)
    loss, dz = NX.ntxent(z, 1.0 / it)
    assert NB.sum_ref(r["row_loss"], M)[0] == pytest.approx(loss, rel=1e-13)
    W = NB.coeff_ref(S, r["lse"], it)["W"]
    assert np.allclose(DPO.normalize_bwd(W @ zh, zh, n), dz, rtol=1e-10, atol=1e-15)
    assert (np.diag(W) == 0).all() and np.allclose(W, W.T, rtol=1e-12, atol=0)


@pytest.mark.parametrize("Ml,world", [(6, 2), (2, 3), (66, 4)])
def test_statements_agree_with_the_sharded_oracle(Ml, world):
    tau = 0.1
    it = NB.f32(1.0 / tau)
    z = NB.make_z("randn", Ml, world).astype(F32)
    shards = [z[r * Ml:(r + 1) * Ml] for r in range(world)]
    loss, dz, lses = DPO.ntxent_sharded(shards, 1.0 / it)
    zh_all = NX.normalize(z)[0]
    lse_all = np.concatenate(lses)
    total = 0.0
    for r in range(world):
        S = zh_all[r * Ml:(r + 1) * Ml] @ zh_all.T
        Sx = S.copy()
        Sx[np.arange(Ml), r * Ml + np.arange(Ml)] = np.nan              # excluded means never used
        ref = NB.rows_ref(Sx, it, Ml * world, r * Ml)
        assert np.allclose(ref["lse"], lses[r], rtol=1e-13)
        total += ref["row_loss"].sum()
        W = NB.coeff_rect_ref(S, lses[r], lse_all, r * Ml, it)["W"]
        zh, n = NX.normalize(shards[r])
        assert np.allclose(DPO.normalize_bwd(W @ zh_all, zh, n), dz[r], rtol=1e-10, atol=1e-15)
    assert total / (Ml * world) == pytest.approx(loss, rel=1e-13)


@pytest.mark.parametrize("M", [6, 66, 258])
@pytest.mark.parametrize("tau", NB.TAUS)
def test_known_answers_of_a_collapsed_batch(M, tau):
    """S = 1 everywhere: lse = inv_tau + log(M - 1), loss = log(M - 1), W_ij = scale (2 / (M - 1) - pair terms)."""
    it = NB.f32(1.0 / tau)
    S = NB.poison(NB.make_S("collapsed", M))
    r = NB.rows_ref(S, it)
    assert np.allclose(r["lse"], it + math.log(M - 1), rtol=1e-14)
    assert NB.sum_ref(r["row_loss"], M)[0] == pytest.approx(math.log(M - 1), rel=1e-12)
    W = NB.coeff_ref(S, r["lse"], it, 0.25)["W"]
    i = np.arange(M)
    pair = np.zeros((M, M))
    pair[i, NB.positives(M)] = 2.0
    want = 0.25 * it / M * (2.0 / (M - 1) - pair)
    want[i, i] = 0.0
    assert np.allclose(W, want, rtol=1e-11, atol=1e-15)


@pytest.mark.parametrize("family", NB.FAMILIES)
def test_known_answers_of_two_rows(family):
    """M = 2: one term in every log-sum-exp, so loss = 0 exactly and W = 0 everywhere."""
    S = NB.poison(NB.make_S(family, 2))
    r = NB.rows_ref(S, 10.0)
    assert (r["row_loss"] == 0.0).all() and NB.sum_ref(r["row_loss"], 2)[0] == 0.0
    assert (NB.coeff_ref(S, r["lse"], 10.0)["W"] == 0.0).all()
    r = NB.rows_ref(NB.poison(NB.make_S(family, 2, 3)[2:4], 2), 10.0, 6, 2)
    assert np.isfinite(r["lse"]).all()


def test_families_are_what_they_claim():
    S = NB.make_S("asym", 66)
    assert np.abs(S - S.T).mean() > 0.3
    for Ml, world in ((6, 1), (6, 2), (2, 3), (34, 2)):
        Mg = Ml * world
        S = NB.make_S("duplicates", Ml, world)
        i = np.arange(Mg)
        pos = np.concatenate([NB.positives(Ml, r0) for r0 in range(0, Mg, Ml)])
        twin = (np.isclose(S, 1.0, atol=1e-6) & (i[:, None] != i[None, :]) & (i[None, :] != pos[:, None])).any(1)
        assert twin.all(), (Ml, world)
        assert (NB.make_S("onehot", Ml, world)[i, pos] == 1.0).all() and (NB.make_S("antipodal", Ml, world)[i, pos] == -1.0).all()
        Z = NB.make_S("zero_rows", Ml, world)
        assert (Z[1 % Mg] == 0).all() and (Z[:, Mg - 2] == 0).all()
    assert NB.f32(math.exp(-100.0)) < 1.2e-38                            # onehot at tau = 0.01: the other terms are fp32 subnormals


# ------------------------------------------------------------------------------------------ the emulation inside the bounds
def square_ratios(v, M, tau, pads, gscale, mutant=None):
    """The emulated rows, sum and coeff kernels on one input: ratio per output."""
    family, fill = NB.variant(v)
    it = NB.f32(1.0 / tau)
    lds, ldw = M + pads[0], M + pads[1]
    S = NB.poison(NB.make_S(family, M), 0, lds, fill)
    lse, row_loss, out = NB.emulate_rows(S, lds, M, M, 0, it, M, mutant)
    r = NB.judge_rows(lse, row_loss, out, S, it, M, 0, M)
    lse_in = lse if np.isfinite(lse).all() else NB.rows_ref(S, it, M)["lse"].astype(F32)
    flat = NB.emulate_coeff(S, lds, lse_in, M, it, gscale, ldw, mutant)
    r["W"] = NB.judge_w(flat[:M * ldw], M, M, ldw, NB.coeff_ref(S, lse_in, it, 1.0, M), gscale)
    if not NB.split_w(flat, M, M, ldw)[1]:
        r["W"] = math.inf
    return r


def rect_ratios(v, Ml, world, row0, tau, pads, gscale, mutant=None):
    family, fill = NB.variant(v)
    it = NB.f32(1.0 / tau)
    Mg = Ml * world
    lds, ldw = Mg + pads[0], Mg + pads[1]
    Sg = NB.make_S(family, Ml, world)
    S = NB.poison(Sg[row0:row0 + Ml], row0, lds, fill)
    lse, row_loss, out = NB.emulate_rows(S, lds, Ml, Mg, row0, it, 1.0, mutant)
    r = {k + "_rect": x for k, x in NB.judge_rows(lse, row_loss, out, S, it, Mg, row0, 1.0).items()}
    lse_in = lse if np.isfinite(lse).all() else NB.rows_ref(S, it, Mg, row0)["lse"].astype(F32)
    lse_all = NB.lse_all_for(Sg, Ml, it)
    flat = NB.emulate_coeff_rect(S, lds, lse_in, lse_all, Ml, Mg, row0, it, gscale, ldw, mutant)
    r["W_rect"] = NB.judge_w(flat, Ml, Mg, ldw, NB.coeff_rect_ref(S, lse_in, lse_all, row0, it), gscale)
    return r


@pytest.mark.parametrize("M", NB.SQUARE_M)
def test_emulation_stays_inside_the_square_bounds(M):
    for k, tau in enumerate(NB.TAUS):
        for n, v in enumerate(NB.VARIANTS):
            pads = ((0, 0), (NB.LDS_PAD, NB.LDW_PAD))[(k + n) % 2]
            r = square_ratios(v, M, tau, pads, NB.GSCALES[(k + n // 2) % 2])
            print(f"NTXENT-BOUNDS emulated {v} M={M} tau={tau}: " + " ".join(f"{a}={b:.4f}" for a, b in r.items()))
            assert all(note(a, b) <= 1.0 for a, b in r.items()), (v, M, tau, r)


@pytest.mark.parametrize("Ml,world", NB.RECT)
def test_emulation_stays_inside_the_rectangular_bounds(Ml, world):
    for k, tau in enumerate(NB.TAUS):
        for n, v in enumerate(NB.VARIANTS):
            for row0 in range(0, Ml * world, Ml):
                pads = ((0, 0), (NB.LDS_PAD, NB.LDW_PAD))[(k + n) % 2]
                r = rect_ratios(v, Ml, world, row0, tau, pads, NB.GSCALES[(k + n // 2) % 2])
                assert all(note(a, b) <= 1.0 for a, b in r.items()), (v, Ml, world, row0, tau, r)
    print(f"NTXENT-BOUNDS emulated rect Ml={Ml} world={world}: " + " ".join(f"{a}={b:.4f}" for a, b in WORST.items() if a.endswith("_rect")))


def test_world_one_is_the_square_kernel_bit_for_bit():
    for M in (6, 258):
        S = NB.poison(NB.make_S("randn", M))
        a, b = NB.emulate_rows(S, M, M, M, 0, 10.0, M), NB.emulate_rows(S, M, M, M, 0, 10.0, 1.0)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize("M,D", [(6, 5), (66, 32), (258, 384)])
def test_end_to_end_bound_holds_an_fp32_evaluation(M, D):
    """The carried bound on loss and dz against an fp32 evaluation of the whole chain (the emulated kernels between NumPy fp32
    products), square and with S_ij standing in for S_ji."""
    for family in NB.E2E_FAMILIES:
        for tau in NB.E2E_TAUS:
            it = NB.f32(1.0 / tau)
            z = NB.make_z(family, M, 1, D).astype(F32)
            n = np.sqrt((z * z).sum(1, dtype=F32))
            zh = (z * (F32(1) / np.maximum(n, F32(1e-12)))[:, None]).astype(F32)
            S = (zh @ zh.T).astype(F32)
            for rect in (False, True):
                ref = NB.e2e_ref(z, it, rect)
                lse, _, out = NB.emulate_rows(S, M, M, M, 0, it, M)
                if rect:
                    W = NB.emulate_coeff_rect(S, M, lse, lse, M, M, 0, it, 1.0, M).reshape(M, M)
                else:
                    W = NB.split_w(NB.emulate_coeff(S, M, lse, M, it, 1.0, M), M, M, M)[0]
                g = (W @ zh).astype(F32)
                cl = n < F32(1e-12)
                dot = np.where(cl, F32(0), (g * zh).sum(1, dtype=F32))
                dz = ((g - zh * dot[:, None]) * (F32(1) / np.where(cl, F32(1e-12), n))[:, None]).astype(F32)
                rl = NB.check(out, ref["loss"], ref["loss_bound"])["ratio"]
                rd = NB.check(dz, ref["dz"], ref["dz_bound"])
                print(f"NTXENT-BOUNDS emulated e2e{'_rect' if rect else ''} {family} {M}x{D} tau={tau}: loss={rl:.4f} dz={rd['ratio']:.4f}")
                assert rd["nan"] == 0 and note("e2e.loss", rl) <= 1.0 and note("e2e.dz", rd["ratio"]) <= 1.0, (family, tau, rect, rl, rd)


# ------------------------------------------------------------------------------------------ the planted defects
SQUARE_PROBES = [(v, M, 0.1, pads) for M in (6, 34, 258) for v in ("randn", "asym") for pads in ((0, 0), (NB.LDS_PAD, NB.LDW_PAD))]
RECT_PROBES = [("randn", 6, 2, 6), ("asym", 66, 4, 132), ("randn", 2, 3, 2)]


@pytest.mark.parametrize("mutant", NB.MUTANTS)
def test_every_planted_defect_leaves_a_bound(mutant):
    """Each on cases of the GPU list (randn and asym at M = 6, 34, 258 and 1026 rows for the sum; three rank blocks with row0 > 0)."""
    caught = []
    for v, M, tau, pads in SQUARE_PROBES:
        r = square_ratios(v, M, tau, pads, 1.0, mutant)
        caught += [f"{k} {v} M={M} pads={pads} {x:.3g}" for k, x in r.items() if x > 1.0]
    for v, Ml, world, row0 in RECT_PROBES:
        r = rect_ratios(v, Ml, world, row0, 0.1, (NB.LDS_PAD, NB.LDW_PAD), 1.0, mutant)
        caught += [f"{k} {v} {Ml}x{Ml * world} row0={row0} {x:.3g}" for k, x in r.items() if x > 1.0]
    if mutant == "sum_second_pass_dropped":
        S = NB.poison(NB.make_S("randn", 1026))
        lse, row_loss, out = NB.emulate_rows(S, 1026, 1026, 1026, 0, 10.0, 1026, mutant)
        r = NB.judge_rows(lse, row_loss, out, S, 10.0, 1026, 0, 1026)
        assert r["lse"] <= 1.0 and r["row_loss"] <= 1.0
        caught += [f"{k} randn M=1026 {x:.3g}" for k, x in r.items() if x > 1.0]
    print(f"NTXENT-BOUNDS mutant {mutant}: {len(caught)} outputs outside, e.g. {caught[:3]}")
    assert caught, mutant


def test_what_the_old_bar_let_through():
    """The issue's example: at M = 260 a column dropped from every log-sum-exp moves the mean loss by far less than 1e-3 relative,
    and every lse by hundreds of bounds."""
    M, it = 260, 10.0
    S = NB.poison(NB.make_S("randn", M))
    good, bad = NB.emulate_rows(S, M, M, M, 0, it, M), NB.emulate_rows(S, M, M, M, 0, it, M, "last_col_dropped")
    assert abs(float(bad[2]) - float(good[2])) < 1e-3 * abs(float(good[2]))
    assert NB.judge_rows(*bad, S, it, M, 0, M)["lse"] > 10.0 and NB.judge_rows(*good, S, it, M, 0, M)["lse"] <= 1.0


def test_zz_report_error_to_bound_ratios():
    for k in sorted(WORST):
        print(f"NTXENT-BOUNDS emulated max {k}: ratio={WORST[k]:.4f}")
