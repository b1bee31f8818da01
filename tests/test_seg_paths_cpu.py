"""CPU checks of the segmentation path table (tests/_seg_paths_cases.py): the table reaches every compiled path of the seg family and
needs each of its cases; its mirror of the host dispatch agrees with the sources read as text; every new case stays inside the caps the
arg-max comparisons of the existing modules keep (tests/test_segloss_gpu.py::test_predict and tests/test_segcalib_gpu.py: at most 1 % of
the pixels undecided, held here for every loss case; tests/test_segrefine_cpu.py: 1 %; tests/_segblend_oracle.Blend.check: 1e-3); and the float64
oracles take u = 1, 24, 32 and C = 32 with finite, positive bounds.

The inputs and the oracle objects of every case are built here, once, and tests/test_seg_paths_gpu.py takes them from here."""
import os
import re
from functools import lru_cache

import numpy as np
import pytest

import _bdloss_oracle as BO
import _seg_paths_cases as P
import _segblend_oracle as BLO
import _segcalib_oracle as CO
import _segloss_oracle as SO
import _segrefine_oracle as RO
from conftest import ROOT
from test_segloss_gpu import make_labels, make_logits
from test_segrefine_cpu import normal_case

CSRC = os.path.join(ROOT, "dino-x_amd", "csrc")
SPACING = np.array([[0.7, 1.9], [1.3, 0.6]], dtype=np.float32)      # the non-unit spacing of tests/test_bdloss_gpu.py
ids = lambda cases: [c["name"] for c in cases]


# ------------------------------------------------------------------------------------------ inputs and oracles, once per case
@lru_cache(maxsize=None)
def loss_inputs(name: str):
    """(case, z fp32 [B, g^2, C], y uint8 [B, S, S]) of a loss case; read-only."""
    c = P.BY_NAME["loss", name]
    rng = np.random.default_rng([71, c["g"], c["u"], c["B"], c["C"], c["i"]])
    z = make_logits(rng, c["logits"], c["B"], c["g"] ** 2, c["C"])
    y = make_labels(rng, c["labels"], c["B"], c["g"] * c["u"], c["C"])
    z.setflags(write=False)
    y.setflags(write=False)
    return c, z, y


@lru_cache(maxsize=None)
def loss_oracle(name: str):
    """The per-pixel quantities and the plain forward / backward of a loss case."""
    c, z, y = loss_inputs(name)
    px = SO.Pixels(z, y, c["g"], c["u"])
    fwd = SO.forward(z, y, c["g"], c["u"], *c["weights"], c["c0"], px)
    dz, e_dz = SO.backward(z, y, c["g"], c["u"], *c["weights"], c["c0"], 1.0, px, fwd)
    return px, fwd, dz, e_dz


def bd_oracle(name: str, phi):
    """The boundary pair of a loss case against the phi the kernel reads (fp32 values, [B, C, S, S])."""
    c, z, y = loss_inputs(name)
    px = loss_oracle(name)[0]
    w_ce, w_dice, w_bd = c["triple"]
    fwd = BO.forward(z, y, phi, c["g"], c["u"], w_ce, w_dice, w_bd, c["c0"], px)
    dz, e_dz = BO.backward(z, y, phi, c["g"], c["u"], w_ce, w_dice, w_bd, c["c0"], 1.0, px, fwd)
    return fwd, dz, e_dz


@lru_cache(maxsize=None)
def calib_oracle(name: str):
    c, z, y = loss_inputs(name)
    cal = CO.Calib(z, y, c["g"], c["u"])
    return cal, cal.at(c["s"])


@lru_cache(maxsize=None)
def refine_inputs(name: str):
    """(case, z, guide, y) of a refinement case: the "normal" arrays of tests/test_segrefine_cpu.py."""
    c = P.BY_NAME["refine", name]
    z, guide = normal_case(c["g"], c["u"], c["B"], c["C"], 100 + c["i"])
    y = make_labels(np.random.default_rng([73, c["C"], c["i"]]), P.LABELS[c["i"] % 4], c["B"], c["g"] * c["u"], c["C"])
    return c, z, guide, y


@lru_cache(maxsize=None)
def refine_oracle(name: str):
    c, z, guide, _ = refine_inputs(name)
    return RO.refine(z, guide, c["g"], c["u"], **c["params"])


@lru_cache(maxsize=None)
def blend_case(name: str):
    """(case, geometry, ys, xs, win, z, oracle) of a blend case, as tests/_segblend_cases.case builds its own."""
    import _segblend_cases as K
    from dinox.tiled import blend_window, tile_starts
    c = P.BY_NAME["blend", name]
    H, W, t, g, overlap = K.GEOMETRIES[c["gi"]]
    ys, xs = tile_starts(H, t, overlap), tile_starts(W, t, overlap)
    win = blend_window(t, c["window"])
    z = BLO.make_logits(c["logits"], (c["B"], c["F"], len(ys), len(xs), g * g, c["C"]), c["seed"])
    z.setflags(write=False)
    return c, (H, W, t, g), ys, xs, win, z, BLO.Blend(z, ys, xs, c["flips"], win, H, W, t)


# ------------------------------------------------------------------------------------------ coverage of the table
def test_the_table_reaches_every_path():
    got, full = P.reached_by(P.CASES), P.full_set()
    assert got == full, f"not reached: {sorted(full - got, key=str)}; outside the full set: {sorted(got - full, key=str)}"
    assert {P.width(c["C"]) for c in P.CLASS_CASES} == {4, 8, 16, 32} and all(c["g"] == 3 and c["B"] == 2 for c in P.CLASS_CASES)
    assert {(c["C"], c["params"]["r"]) for c in P.REFINE_CASES} == {(C, r) for C in P.WIDTHS for r in (1, 2, 3)}
    assert all((c["g"], c["u"], c["params"]["d"], c["params"]["T"]) == (3, 8, 2, 2) for c in P.REFINE_CASES)
    # 18 cells: three parts of SEG_FWD_CELLS with a ragged last one and an idle wave beside them; five ragged parts of SEG_CALIB_CELLS
    assert P.ragged_parts(2, 3, P.SEG_FWD_CELLS) == (3, 2, 1) and P.ragged_parts(2, 3, P.SEG_CALIB_CELLS) == (5, 2, 3)
    for c in P.CASES:
        assert c["path"] and c.get("B", 1) <= 2 and c.get("g", 1) * c.get("u", 1) <= 96


@pytest.mark.parametrize("case", P.CASES, ids=lambda c: f"{c['kind']}-{c['name']}")
def test_every_case_is_needed(case):
    """Without this case a path of the full set is reached by nothing else: the path it is in the table for."""
    rest = P.reached_by(c for c in P.CASES if c is not case)
    lost = P.full_set() - rest
    assert lost, f"{case['name']} ({case['path']}) reaches nothing the other cases do not"
    assert lost <= P.reached(case)


def test_the_required_cell_widths_occur():
    for u, ws in P.FACTOR_WIDTHS.items():
        assert {cw for cw, _ in P.cell_widths(3, u)} == set(ws)
        assert all(R == 64 // cw for cw, R in P.cell_widths(3, u))
    assert P.cell_widths(3, 24) == {(36, 1), (24, 2), (12, 5)}                    # 28, 16 and 4 dead lanes
    assert P.cell_widths(1, 32) == {(32, 2)} and P.cell_widths(2, 8) == {(12, 5), (4, 16)}
    for u in P.ACCESS_FACTORS:                                                     # what the four-lane pack rests on
        assert all(cw % 4 == 0 for cw, _ in P.cell_widths(3, u)) and all(P.lo(k, 3, u) % 4 == 0 for k in range(4))


# ------------------------------------------------------------------------------------------ the mirror against the sources
def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_the_mirror_agrees_with_the_sources():
    common, loss, calib, blend = _src("seg_common.h"), _src("segloss.hip"), _src("segcalib.hip"), _src("segblend.hip")
    cp = re.search(r"static int seg_cp\(int C\) \{ return (.*?); \}", common).group(1)
    assert [(int(a), int(b)) for a, b in re.findall(r"C <= (\d+) \? (\d+)", cp)] == [(t, t) for t in P.CP_THRESHOLDS] and cp.endswith(": 64")
    by_width = common[common.index("seg_by_width(int C"):common.index("the cell walk")]
    assert tuple(int(v) for v in re.findall(r"integral_constant<int, (\d+)>", by_width)) == P.WIDTHS
    for C in range(2, 65):
        assert P.width(C) == next((t for t in P.CP_THRESHOLDS if C <= t), 64) and P.width(C) >= C
    assert int(re.search(r"constexpr int SEG_FWD_CELLS = (\d+);", loss).group(1)) == P.SEG_FWD_CELLS
    assert int(re.search(r"constexpr int SEG_CALIB_CELLS = (\d+);", calib).group(1)) == P.SEG_CALIB_CELLS
    assert int(re.search(r"constexpr int SEG_MAX_UPSAMPLE = (\d+);", common).group(1)) == P.SEG_MAX_UPSAMPLE == max(P.FACTOR_WIDTHS)
    assert int(re.search(r"constexpr int SEG_WAVES = (\d+);", common).group(1)) == P.SEG_WAVES
    sw = re.search(r"static int seg_wide\(const void\* p, int u\) \{ return (.*?); \}", common).group(1)
    assert sw == "u % 8 == 0 && (reinterpret_cast<uintptr_t>(p) & 3) == 0"
    assert [P.wide(o, u) for u in (8, 12, 24) for o in range(4)] == [True, False, False, False] + [False] * 4 + [True, False, False, False]
    assert "return k <= 0 ? 0 : (k >= g ? S : k * u + u / 2);" in common and "R = 64 / cw" in common      # seg_lo, the rows of a wave
    assert "const int pwide = W % 4 == 0 && (reinterpret_cast<uintptr_t>(pred) & 3) == 0;" in blend and "if (C == CP) {" in blend
    import _segblend_cases as K
    assert all(K.GEOMETRIES[gi] == P.blend_geometry(gi) for gi in P.BLEND_GEOMETRIES)
    # the refinement kernel's radii and its tile (S = 24: one ragged tile across, three down)
    refine = _src("segrefine.hip")
    assert re.search(r"SEG_REFINE_TW = (\d+), SEG_REFINE_TH = (\d+)", refine).groups() == ("32", "8")
    assert [int(v) for v in re.findall(r"go\(std::integral_constant<int, (\d)>\{\}\)", refine)] == [1, 2, 3]


# ------------------------------------------------------------------------------------------ the conditions of the arg-max comparisons
@pytest.mark.parametrize("case", P.LOSS_CASES, ids=lambda c: c["name"])
def test_undecided_share_of_the_loss_cases(case):
    """The cap of test_predict and of the calibration tests, for every loss case whatever its logits: at most 1 % of the pixels have a
    float64 top-two margin under the bound, so the arg-max comparisons of the GPU module see (nearly) every pixel."""
    _, z, _ = loss_inputs(case["name"])
    _, margin, e_l = SO.predict(z, case["g"], case["u"])
    share = 1.0 - (margin > e_l).mean()
    twice = 1.0 - (margin > 2 * e_l).mean()                 # the rule of the refinement oracle, which T = 0 is held to
    print(f"{case['name']}: {share:.2%} of {margin.size} pixels undecided ({twice:.2%} under twice the bound)")
    assert share <= 0.01 and twice <= 0.01


@pytest.mark.parametrize("case", P.REFINE_CASES, ids=lambda c: c["name"])
def test_undecided_share_of_the_refine_cases(case):
    o = refine_oracle(case["name"])
    share = 1.0 - o["decided"].mean()
    print(f"{case['name']}: {share:.2%} of {o['decided'].size} pixels undecided")
    assert o["finite"].all() and share <= 0.01
    assert np.isfinite(o["e_conf"]).all() and (o["e_conf"] > 0).all() and (o["e_conf"] < 1e-3).all() and (o["e_V"] > 0).all()


@pytest.mark.parametrize("case", P.BLEND_CASES, ids=lambda c: c["name"])
def test_exempt_share_of_the_blend_cases(case):
    """The cap of Blend.check (1e-3), on the oracle alone and on its fp32 emulation of the kernel."""
    c, (H, W, t, g), ys, xs, win, z, want = blend_case(case["name"])
    share = 1.0 - want.decided.mean()
    print(f"{case['name']}: exempt share {share:.2e} of {want.decided.size} pixels")
    assert share <= 1e-3
    assert np.isfinite(want.e_L).all() and (want.e_L > 0).all() and np.isfinite(want.e_conf).all() and (want.e_conf > 0).all()
    want.check(*BLO.emulate(z, ys, xs, c["flips"], win, H, W, t))


# ------------------------------------------------------------------------------------------ the oracles at the new shapes
def _sane(name, bound, ref):
    bound, ref = np.asarray(bound, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert np.isfinite(bound).all() and np.isfinite(ref).all() and (bound >= 0).all(), name
    assert (bound[ref != 0] > 0).all(), f"{name}: a zero bound on a non-zero value"


def host_phi(y, spacing, C):
    """BO.signed_distance's values by rows: min over source rows r of (s_y (Y - r))^2 + min over the row's sources of (s_x (X - x))^2, the
    root taken last -- the same float64 expressions over the same pairs (the root is monotone), at S^3 instead of S^4 per class, so that
    the 96 x 96 cases stay at a second here.  Held to the brute force below."""
    y = np.asarray(y)
    B, H, W = y.shape
    sp = np.asarray(spacing, dtype=np.float32).astype(np.float64).reshape(B, 2)
    phi = np.zeros((B, C, H, W))
    for b in range(B):
        dx2 = (sp[b, 1] * (np.arange(W)[:, None] - np.arange(W)[None, :])) ** 2      # [X, x]
        dy2 = (sp[b, 0] * (np.arange(H)[:, None] - np.arange(H)[None, :])) ** 2      # [Y, r]
        valid = y[b] != BO.IGNORE

        def nearest(mask):                                   # [H, W]: distance to the nearest pixel of the mask
            row = np.where(mask[:, None, :], dx2[None], np.inf).min(-1)              # [r, X]
            return np.sqrt((dy2[:, :, None] + row[None]).min(1))

        for c in range(C):
            G, R = y[b] == c, valid & (y[b] != c)
            if G.any() and R.any():
                phi[b, c] = np.where(R, nearest(G), np.where(G, -nearest(R), 0.0))
    return phi


def test_host_phi_is_the_brute_force():
    _, _, y = loss_inputs("g3u8")
    assert np.array_equal(host_phi(y, SPACING, 24), BO.signed_distance(y, SPACING, 24))
    y = np.array(loss_inputs("g2u8")[2])
    y[0, :, 3], y[1, 5:9, 2:11] = 255, 4
    assert np.array_equal(host_phi(y, SPACING, 13), BO.signed_distance(y, SPACING, 13))


@pytest.mark.parametrize("case", P.LOSS_CASES, ids=lambda c: c["name"])
def test_oracle_bounds_of_the_loss_cases(case):
    c, z, y = loss_inputs(case["name"])
    px, fwd, dz, e_dz = loss_oracle(case["name"])
    assert fwd["nv"] > 0 and (px.e_l > 0).any()
    _sane("loss", fwd["e_loss"], fwd["loss"])
    _sane("stats", fwd["e_stats"][:2], fwd["stats"][:2])    # (the label counts are integers: compared exactly)
    _sane("dz", e_dz, dz)
    assert e_dz.max() > 0 or not any(c["weights"])
    phi = host_phi(y, SPACING[:c["B"]], c["C"]).astype(np.float32)
    bfwd, bdz, e_bdz = bd_oracle(case["name"], phi)
    _sane("bd loss", bfwd["e_loss"], bfwd["loss"])
    _sane("bd dz", e_bdz, bdz)
    cal, o = calib_oracle(case["name"])
    _sane("conf", o["e_conf"], o["conf"])
    _sane("entropy", o["e_entropy"], o["entropy"])
    _sane("sums", o["e_sums"], o["sums"])
    assert (o["e_conf"] > 0).all() and o["nv"] == fwd["nv"]
