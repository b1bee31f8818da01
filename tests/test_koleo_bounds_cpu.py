"""The elementwise KoLeo bounds of oracle/koleo_bounds.py, checked without a GPU against the NumPy fp32 emulation of
tests/_koleo_emul.py (the kernels' summation shape and the chunks of the ballot compaction):

  * the fault-free emulation stays at or below 0.75 x every bound on every family, and its indices are exactly the required ones;
  * each planted defect is flagged on a NAMED family or case;
  * randn rows at 96 rows, all the suite had, miss the expanded-form distance, the restarted chunk offsets and (d + eps)^2;
  * the planted pairs of the `pairs` family are decided by the float64 reference alone, by more than 2 e_sel;
  * every DX_REQUIRE of the five entry points refuses with its message (host only, fake pointers).
"""
import ctypes as C

import numpy as np
import pytest

import _koleo_emul as E
import _small_kernels_oracle as SO
from oracle import koleo_bounds as KB

MARGIN = 0.75
F32 = np.float32


def ratio(got, ref, bound):
    c = KB.check(got, ref, bound)
    assert c["nan"] == 0, c
    return c["ratio"]


def normalize_ratios(x, defect=None):
    xh, norm, sq = E.normalize(x, defect=defect)
    r = KB.normalize_ref(x)
    return {k: ratio(v, r[k], r[k + "_bound"]) for k, v in (("xh", xh), ("norm", norm), ("sq", sq))}, (xh, norm, sq), r


def nn_case(V_l, V_g, row0, D=16, seed=0):
    xh = KB.unit_rows(V_g, D, seed)
    return KB.gram32(xh[row0:row0 + V_l], xh), KB.sq32(xh), xh


def nn_ratio(G, sq, xh, row0, defect=None, want=None):
    """(indices exact?, distance ratio) of the emulated search."""
    idx, dist = E.nn(G, sq, xh, row0, defect=defect)
    want = KB.nn_index(G, sq, row0) if want is None else want
    ref, bound = KB.nn_dist_ref(xh, want, row0)
    return bool((idx == want).all()), KB.check(dist, ref, bound)["ratio"]


def bwd_ratio(c, defect=None):
    ref = KB.bwd_ref(c["xh_all"], c["idx_all"], c["dist_all"], c["norm_loc"], c["row0"], c["gscale"])
    got = E.bwd(c["xh_all"], c["idx_all"], c["dist_all"], c["norm_loc"], c["row0"], c["gscale"], defect=defect)
    return KB.check(got, ref["dx"], ref["dx_bound"])["ratio"], ref


def e2e_ratios(x, defect=None):
    """Every stage of the emulated chain judged given what the stage before it produced."""
    o = E.end_to_end(x, defect=defect)
    V = len(x)
    out, _, _ = normalize_ratios(x, defect)
    want = KB.nn_index(o["G"], o["sq"], 0)
    ref, bound = KB.nn_dist_ref(o["xh"], want, 0)
    out["idx_exact"] = bool((o["idx"] == want).all())
    out["dist"] = KB.check(o["dist"], ref, bound)["ratio"]
    l, le = KB.loss_ref(o["dist"], log_rtol=SO.CE_LOSS_RTOL)
    out["loss"] = abs(float(o["loss"]) - l) / le
    b = KB.bwd_ref(o["xh"], o["idx"], o["dist"], o["norm"], 0, 1.0 / V)
    out["dx"] = KB.check(o["dx"], b["dx"], b["dx_bound"])["ratio"]
    return out, o


# ------------------------------------------------------------------------------------------ the selection value
@pytest.mark.parametrize("family", KB.FAMILIES)
def test_selection_value_is_one_number_with_or_without_fma(family):
    """2 G is exact, so fl(s - fl(2 G)) and the fused fl(s - 2 G) are the same fp32 number: idx can be required exactly."""
    xh, _, sq = E.normalize(KB.make_rows(family, 96, 40, offset=30.0))
    G = KB.gram32(xh, xh)
    s = (sq[:, None] + sq[None, :]).astype(F32)
    two_g = F32(2.0) * G
    assert (two_g.astype(np.float64) == 2.0 * G.astype(np.float64)).all()
    fused = (s.astype(np.float64) - 2.0 * G.astype(np.float64)).astype(F32)        # the float64 difference of two fp32 numbers of this range is exact
    v = KB.selection_values(G, sq, 0)
    off = ~np.eye(96, dtype=bool)
    assert (fused.view(np.uint32)[off] == v.view(np.uint32)[off]).all()


# ------------------------------------------------------------------------------------------ clean emulation
@pytest.mark.parametrize("D", KB.WIDTHS + (KB.WIDE,))
def test_normalize_within_margin(D):
    for family in KB.FAMILIES:
        r, (xh, norm, sq), ref = normalize_ratios(KB.make_rows(family, 6, D))
        assert max(r.values()) <= MARGIN, (family, D, r)
        if family.startswith("zero"):
            assert (xh[2] == 0).all() and sq[2] == 0 and norm[2] == 0
        if family == "tiny":
            assert ref["clamped"].tolist() == [False, True] + [False] * 4
            assert 0.009 < sq[1] < 0.011 and abs(sq[3] - 1) < 1e-6       # a / eps^2 = (1e-13 / 1e-12)^2 below the clamp, 1 above it


def test_normalize_refuses_a_row_on_the_clamp():
    x = np.zeros((1, 4), dtype=F32)
    x[0, 0] = KB.NORM_EPS
    with pytest.raises(ValueError):
        KB.normalize_ref(x)


@pytest.mark.parametrize("V_l,V_g,row0", [(v, v, 0) for v in KB.NN_SIZES] + list(KB.RECT))
def test_nn_within_margin(V_l, V_g, row0):
    G, sq, xh = nn_case(V_l, V_g, row0)
    exact, r = nn_ratio(G, sq, xh, row0)
    assert exact and r <= MARGIN, (exact, r)
    if V_g == 1:
        idx, dist = E.nn(G, sq, xh, 0)
        assert idx[0] == -1 and dist[0] == KB.NO_NEIGHBOUR and KB.nn_index(G, sq, 0)[0] == -1


@pytest.mark.parametrize("mode", KB.TIE_MODES)
def test_nn_ties_take_the_lowest_index(mode):
    for V_l, V_g, row0 in [(100, 700, 300), (100, 700, 0), (700, 700, 0)]:
        G, sq, want = KB.tie_case(mode, V_l, V_g, row0)
        assert (KB.nn_index(G, sq, row0) == want).all()                  # the float32 rule gives the planted lowest column
        assert (KB.selection_values(G, sq, row0).min(1) == F32(0.5)).all()
        exact, r = nn_ratio(G, sq, KB.unit_rows(V_g, 16), row0, want=want)
        assert exact and r <= MARGIN


@pytest.mark.parametrize("V", KB.LOSS_SIZES)
def test_loss_within_margin(V):
    d = np.abs(np.random.default_rng(V).standard_normal(V)).astype(F32)
    d[0] = 0.0
    d[V // 2] = 0.0 if V == 1 else 1e9
    ref, bound = KB.loss_ref(d, log_rtol=SO.CE_LOSS_RTOL)
    assert abs(float(E.loss(d)) - ref) <= MARGIN * bound


@pytest.mark.parametrize("name", KB.BWD_CASES)
def test_bwd_within_margin(name):
    c = KB.bwd_case(name)
    r, ref = bwd_ratio(c)
    assert r <= MARGIN, (name, r)
    if name.startswith("hub"):
        assert ref["n_in"][0] == c["V_g"] - 1 and (c["V_g"] - 1) % 256 != 0
    if name == "nohits":
        assert ref["n_in"].sum() == 0
    if name == "lanes":
        hits = np.nonzero(c["idx_all"] == 5)[0]
        assert set(hits & 63) == {0, 63} and len(hits) == 2 * 11 - 1     # 700 rows: 11 lanes 0 and 10 lanes 63


@pytest.mark.parametrize("D", KB.NBWD_WIDTHS)
def test_normalize_bwd_within_margin(D):
    dxh, xh, norm = KB.nbwd_case(D)
    for vec in ([True, False] if D % 4 == 0 else [False]):
        ref, bound = KB.normalize_bwd_ref(dxh, xh, norm, vec=vec)
        assert ratio(E.normalize_bwd(dxh, xh, norm, vec=vec), ref, bound) <= MARGIN, (D, vec)
        assert np.abs(ref[1]).max() < 1e-6 * np.abs(ref[0]).max() or D == 1   # dxh parallel to xh: the result is the rounding of xh alone


@pytest.mark.parametrize("V,D", KB.E2E + ((96, 64),))
@pytest.mark.parametrize("family", KB.E2E_FAMILIES)
def test_end_to_end_within_margin(family, V, D):
    r, o = e2e_ratios(KB.make_rows(family, V, D, seed=KB.e2e_seed(family, V, D)))
    assert r.pop("idx_exact"), family
    assert max(r.values()) <= MARGIN, (family, r)
    e_sq, e_g = KB.handed_errors(o["xh"], o["xh"], 1)
    c = KB.selection_contract(o["idx"], o["G"], o["sq"], o["xh"], 0, e_sq, e_g)
    assert c["ratio"] <= 1.0, (family, c["ratio"])


# ------------------------------------------------------------------------------------------ what the reference alone decides
@pytest.mark.parametrize("V,D", KB.E2E)
def test_the_reference_alone_decides_the_neighbours(V, D):
    """On the library's own G (any summation order over D terms) the float64 nearest row of EVERY row with a direction beats the others
    by more than 2 e_sel in every family but cluster and offset, so a pick that differs from it breaks the selection contract; the planted pairs
    are each other's nearest rows.  In cluster the five rows, and in offset (1e3 x the common vector) nearly all rows, are NOT
    decided: there the contract alone judges the pick.  The cached seeds are the first decisive ones."""
    terms = D + max(1, D // 256)
    for family in KB.E2E_FAMILIES:
        x = KB.make_rows(family, V, D, seed=KB.e2e_seed(family, V, D))
        xh, _, sq = E.normalize(x)
        G = KB.gram32(xh, xh)
        e_sq, e_g = KB.handed_errors(xh, xh, terms)
        c = KB.selection_contract(KB.nn_index(G, sq, 0), G, sq, xh, 0, e_sq, e_g)
        has_direction = (xh != 0).any(1)
        if family == "cluster":
            assert (c["clear"][:5] < 1.0).all() and (c["clear"][5:] > 1.1).all()
            continue
        if family == "offset":                                          # 1e3 x the common vector: hardly a row is decided
            assert (c["clear"] < 1.0).mean() > 0.9 and family in KB.SHARE_EXEMPT
            continue
        assert family not in KB.SHARE_EXEMPT and KB.e2e_seed(family, V, D) == KB.first_decisive_seed(family, V, D)
        assert (c["clear"][has_direction] > 1.1).all(), (family, float(c["clear"][has_direction].min()))
        if family == "pairs":
            for k in range(6):
                assert c["near"][3 * k] == 3 * k + 1 and c["near"][3 * k + 1] == 3 * k
                d = np.sqrt(c["d2"][3 * k, 3 * k + 1])
                assert 0.8 * KB.PAIR_D[k % 3] < d < 1.2 * KB.PAIR_D[k % 3]


# ------------------------------------------------------------------------------------------ planted defects
def flagged_on(defect):
    """(name of the family or case, flagged?) for one planted defect."""
    if defect == "tie_highest":
        G, sq, want = KB.tie_case("three_waves", 100, 700, 300)
        return "ties/three_waves", not nn_ratio(G, sq, KB.unit_rows(700, 16), 300, defect, want)[0]
    if defect == "self_is_i":
        G, sq, want = KB.tie_case("last", 100, 700, 300)
        return "ties/last row0=300", not nn_ratio(G, sq, KB.unit_rows(700, 16), 300, defect, want)[0]
    if defect in ("expanded_dist", "eps_squared", "own_pair_at_zero"):
        family = "dup" if defect == "own_pair_at_zero" else "pairs"
        r, _ = e2e_ratios(KB.make_rows(family, 96, 64), defect)
        return family, max(r["dist"], r["dx"]) > 1.0
    if defect in ("drop_ragged_chunk", "offsets_restart"):
        return "bwd/hub300", bwd_ratio(KB.bwd_case("hub300"), defect)[0] > 1.0
    if defect == "lane63_lost":
        return "bwd/lanes", bwd_ratio(KB.bwd_case("lanes"), defect)[0] > 1.0
    if defect == "project_clamped":
        return "bwd/clamped", bwd_ratio(KB.bwd_case("clamped"), defect)[0] > 1.0
    if defect == "sq_clamped_one":
        return "tiny", normalize_ratios(KB.make_rows("tiny", 6, 64), defect)[0]["sq"] > 1.0
    if defect == "tail_dropped":
        dxh, xh, norm = KB.nbwd_case(257)
        ref, bound = KB.normalize_bwd_ref(dxh, xh, norm, vec=False)
        return "normalize_bwd D=257", KB.check(E.normalize_bwd(dxh, xh, norm, defect=defect), ref, bound)["ratio"] > 1.0
    raise ValueError(defect)


@pytest.mark.parametrize("defect", E.DEFECTS)
def test_planted_defect_is_flagged(defect):
    where, flagged = flagged_on(defect)
    assert flagged, f"{defect} is not flagged on {where}"


def test_randn_at_96_rows_misses_three_defects():
    """What the suite had: randn rows, at most 96 of them, one chunk, no close pair.  Clean and defective runs both pass there."""
    x = KB.make_rows("randn", 96, 64)
    missed = []
    for defect in ("expanded_dist", "offsets_restart", "eps_squared", "tie_highest", "self_is_i"):
        r, _ = e2e_ratios(x, defect)
        if r.pop("idx_exact") and max(r.values()) <= 1.0:
            missed.append(defect)
    assert {"expanded_dist", "offsets_restart", "eps_squared"} <= set(missed), missed


# ------------------------------------------------------------------------------------------ argument contracts of the C entry points
def test_abi_rejects_bad_arguments_without_a_launch():
    """The checks run on the host, ahead of the launch: the pointers below are never dereferenced."""
    from dinox import _lib
    lib = _lib.lib
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    EINVAL, EUNSUPPORTED = -1, _lib.EUNSUPPORTED
    err = _lib.last_error
    assert EUNSUPPORTED == -2

    assert lib.dinox_koleo_normalize(p, p, None, p, 4, 8, 1e-12, None) == EINVAL and "koleo_normalize: null" in err()
    assert lib.dinox_koleo_normalize(p, p, p, p, 0, 8, 1e-12, None) == EINVAL and "V=0 D=8" in err()
    assert lib.dinox_koleo_normalize(p, p, p, p, 1 << 31, 8, 1e-12, None) == EINVAL and "V=2147483648" in err()
    assert lib.dinox_koleo_normalize(p, p, p, p, 4, 0, 1e-12, None) == EINVAL and "D=0" in err()

    nn = lambda row0=0, V_l=4, V_g=8, ldg=8, D=4, G=p, idx=p: lib.dinox_koleo_nn(G, ldg, p, p, row0, V_l, V_g, D, idx, p, None)
    assert nn(G=None) == EINVAL and "koleo_nn: null" in err()
    assert nn(idx=None) == EINVAL and "koleo_nn: null" in err()
    assert nn(V_l=0) == EINVAL and "V_l=0" in err()
    assert nn(V_g=0, V_l=1) == EINVAL and "V_g=0" in err()
    assert nn(row0=-1) == EINVAL and "row0=-1" in err()
    assert nn(row0=5) == EINVAL and "row0=5 V_l=4 V_g=8" in err()      # the local rows run past the global ones
    assert nn(ldg=7) == EINVAL and "ldg=7" in err()
    assert nn(D=0) == EINVAL and "D=0" in err()

    assert lib.dinox_koleo_loss(None, 4, 1e-8, p, None) == EINVAL and "koleo_loss: null" in err()
    assert lib.dinox_koleo_loss(p, 4, 1e-8, None, None) == EINVAL and "koleo_loss: null" in err()
    assert lib.dinox_koleo_loss(p, 0, 1e-8, p, None) == EINVAL and "koleo_loss: V=0" in err()

    bwd = lambda row0=0, V_l=4, V_g=8, D=4, x=p, dx=p: lib.dinox_koleo_bwd(x, p, p, p, row0, V_l, V_g, D, 1.0, 1e-8, 1e-12, dx, None)
    assert bwd(x=None) == EINVAL and "koleo_bwd: null" in err()
    assert bwd(dx=None) == EINVAL and "koleo_bwd: null" in err()
    assert bwd(V_l=0) == EINVAL and "V_l=0" in err()
    assert bwd(V_g=0, V_l=1) == EINVAL and "V_g=0" in err()
    assert bwd(row0=-1) == EINVAL and "row0=-1" in err()
    assert bwd(row0=6) == EINVAL and "row0=6 V_l=4 V_g=8" in err()
    assert bwd(D=0) == EINVAL and "D=0" in err()
    assert bwd(V_l=2, V_g=KB.MAX_LIST_ROWS + 1) == EUNSUPPORTED and "15360 rows exceeds the neighbour list (15359 rows)" in err()

    nb = lambda V=4, D=8, eps=1e-12, norm=p: lib.dinox_normalize_bwd(p, p, norm, p, V, D, eps, None)
    assert nb(norm=None) == EINVAL and "normalize_bwd: null" in err()
    assert nb(V=0) == EINVAL and "V=0" in err()
    assert nb(V=1 << 31) == EINVAL and "V=2147483648" in err()
    assert nb(D=0) == EINVAL and "D=0" in err()
    assert nb(eps=0.0) == EINVAL and "eps=0" in err()
