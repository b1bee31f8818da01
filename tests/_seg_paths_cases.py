"""The case table of tests/test_seg_paths_gpu.py and a pure-Python mirror of the host dispatch of the dense-segmentation kernels
(csrc/seg_common.h: seg_cp / seg_by_width, seg_wide, the cell geometry of seg_cell_pixels; csrc/segblend.hip: the ``C == CP`` branch and
the packed store).  No GPU, no library call, no NumPy: tests/test_seg_paths_cpu.py computes from the mirror which compiled paths the table
reaches, holds that set to the full one, and holds the mirror to the sources read as text.

Every case names the path it is the smallest shape of (``path``); ``reached(case)`` is what the mirror says it runs.  The inputs are the
generators of the existing modules (make_labels / make_logits of tests/test_segloss_gpu.py, normal_case / make_guide of
tests/test_segrefine_cpu.py, make_logits of tests/_segblend_oracle.py): no new input family.  Images are at most 96 x 96, B <= 2."""

# ------------------------------------------------------------------------------------------ the mirror
WIDTHS = (4, 8, 16, 32, 64)                       # seg_by_width's instantiations
CP_THRESHOLDS = (4, 8, 16, 32)                    # seg_cp: C <= 4 ? 4 : C <= 8 ? 8 : C <= 16 ? 16 : C <= 32 ? 32 : 64
SEG_FWD_CELLS = 8                                 # csrc/segloss.hip
SEG_CALIB_CELLS = 4                               # csrc/segcalib.hip
SEG_MAX_UPSAMPLE = 32                             # csrc/seg_common.h
SEG_WAVES = 4


def width(C: int) -> int:
    """seg_cp: the register width that holds C classes."""
    for t in CP_THRESHOLDS:
        if C <= t:
            return t
    return 64


def wide(offset_bytes: int, u: int) -> bool:
    """seg_wide: the 32-bit label load / packed prediction store, for a pointer ``offset_bytes`` past a 4-byte boundary."""
    return u % 8 == 0 and offset_bytes % 4 == 0


def lo(k: int, g: int, u: int) -> int:
    """seg_lo: the first pixel of cell index k along one axis."""
    return 0 if k <= 0 else (g * u if k >= g else k * u + u // 2)


def cell_widths(g: int, u: int):
    """The set of (cw, R = 64 // cw) over the cells of one axis: the first cell u + u / 2 wide, an interior one u, the last u - u / 2."""
    return {(lo(k + 1, g, u) - lo(k, g, u), 64 // (lo(k + 1, g, u) - lo(k, g, u))) for k in range(g)}


def ragged_parts(B: int, g: int, per: int):
    """(parts, cells of the last part, idle waves of the last workgroup) of B g^2 cells taken ``per`` to a wave."""
    ncell = B * g * g
    parts = -(-ncell // per)
    return parts, ncell - (parts - 1) * per, -parts % SEG_WAVES


# ------------------------------------------------------------------------------------------ what the rotations draw from (the existing modules' lists)
LABELS = ("random", "one class", "absent class", "quarter ignored")      # "all ignored" runs beside every case: exact zeros
LOGITS = ("normal", "dominant")                                          # (not "pm80": see FACTOR_CASES)
WEIGHTS = ((1.0, 1.0), (0.0, 1.0), (1.0, 0.0))                           # (w_ce, w_dice) of the plain pair
TRIPLES = ((1.0, 1.0, 0.5), (0.0, 0.0, 1.0), (0.7, 1.3, 0.25))           # (w_ce, w_dice, w_bd) of the boundary pair, w_bd != 0
NBS = (1, 10, 15, 64)
SS = (1.0, 0.37, 2.5)

LOSS_KERNELS = ("seg_fwd_partial", "seg_fwd_partial<BD>", "seg_bwd_cells", "seg_bwd_cells<BD>", "seg_predict", "seg_calib")
CLASS_ENDS = (4, 8, 9, 16, 17, 32)                # both ends of widths 16 and 32, the exact fills of widths 4 and 8
FACTOR_WIDTHS = {1: (1,), 2: (3, 2, 1), 8: (12, 8, 4), 24: (36, 24, 12), 32: (48, 32, 16)}
ACCESS_FACTORS = (8, 24, 32)


def _loss(name, path, g, u, C, i, logits, labels=None, B=2):
    return dict(kind="loss", name=name, path=path, g=g, u=u, B=B, C=C, i=i, labels=labels or LABELS[i % 4], logits=logits, c0=i % 2, weights=WEIGHTS[i % 3],
                triple=TRIPLES[(i + 1) % 3], NB=NBS[i % 4], s=SS[i % 3], zoff=(i // 2) % 2)


# Class counts: g = 3 (a first, an interior and a last cell on both axes), B = 2 (a non-zero image offset; 18 cells = three ragged parts of
# SEG_FWD_CELLS, five of SEG_CALIB_CELLS, one idle wave in the last workgroup), u = 4 (cells 6 / 4 / 2 wide: dead lanes at 6).  "normal"
# logits throughout: under a dominant class an error at the last class would sit under a probability of e^-40.  No "one class" labels:
# their distance maps are zero planes, and the boundary term would multiply zeros at the widths it has never run at.
CLASS_CASES = [_loss(f"C{C}", f"C = {C}: {'the exact fill' if C == width(C) else 'the low end'} of width {width(C)}", 3, 4, C, i, "normal",
                     ("random", "quarter ignored", "absent class")[i % 3])
               for i, C in enumerate(CLASS_ENDS)]

# Factors: every cell width of FACTOR_WIDTHS at g = 3; g = 1 and 2 at u = 8 and 32 have no interior cell and every second tap clamped
# (g = 1: both).  The class counts stay off CLASS_ENDS (so that each case of the table is needed) and meet widths 16 and 32 at the wide
# factors; 33 and 64 bring width 64 into this table.  The order puts the "one class" labels (zero distance maps) on the two g = 1 cases.
# Logits: "normal" and "dominant" only.  Every loss case also runs seg_predict, seg_calib's pred / conf and the T = 0 refinement against
# the float64 arg-max, which is compared where the margin decides; under "pm80" several classes of a patch sit at +80 together and most
# pixels are exact ties (75 to 100 % undecided at these shapes), so those comparisons would be empty.  tests/test_seg_paths_cpu.py holds
# every loss case to the 1 % cap.
_F = ((3, 24, 12, "normal"), (3, 8, 24, "normal"), (3, 32, 20, "dominant"), (1, 8, 31, "dominant"), (3, 2, 33, "normal"), (3, 1, 64, "normal"),
      (2, 8, 13, "normal"), (1, 32, 10, "dominant"), (2, 32, 3, "normal"))
FACTOR_CASES = [_loss(f"g{g}u{u}", (f"u = {u}: cells {' / '.join(str(w) for w in FACTOR_WIDTHS[u])} wide" if g == 3 else
                                     f"g = {g}, u = {u}: no interior cell, the second tap clamped"), g, u, C, 6 + i, log)
                for i, (g, u, C, log) in enumerate(_F)]
LOSS_CASES = CLASS_CASES + FACTOR_CASES

# Access paths: the g = 3 factor case of each u % 8 == 0 through the C entry points with explicit pointers.  ``yoff`` / ``poff``: bytes
# past a 4-byte boundary of the labels / the prediction map.  (0, 0) is the wide pair, the other the byte pair at a factor where wide is
# the default; the two runs of a factor are compared with each other.
ACCESS_CASES = [dict(kind="access", name=f"u{u}-y{yoff}-p{poff}", of=f"g3u{u}", u=u, yoff=yoff, poff=poff,
                     path=f"u = {u}: {'32-bit label load, packed store' if yoff == 0 else 'byte label load, byte store'}")
                for u, odd in ((8, 1), (24, 3), (32, 1)) for yoff, poff in ((0, 0), (odd, 2))]

# Refinement: every (CP, r) of seg_refine_iter_kernel.  S = 24 is one ragged 32-wide tile by three 8-high ones; d = 2; T = 2, so the
# first launch writes a plane and the last one emits.
REFINE_LAMS = (0.8, 1.0, 0.0)
REFINE_WS = (4.0, 20.0)
REFINE_SIGMA_XY = (3.0, 1.5, 6.0)
REFINE_SIGMA_I = (0.5, 0.25, 2.0)
REFINE_CASES = [dict(kind="refine", name=f"C{C}r{r}", path=f"seg_refine_iter_kernel<{C}, {r}>", g=3, u=8, B=2, C=C, i=3 * ci + r - 1,
                     params=dict(T=2, r=r, d=2, lam=REFINE_LAMS[(ci + r) % 3], w=REFINE_WS[(ci + r) % 2], s=SS[(ci + 2 * r) % 3],
                                 sigma_xy=REFINE_SIGMA_XY[(ci + r) % 3], sigma_i=REFINE_SIGMA_I[(2 * ci + r) % 3]))
                for ci, C in enumerate(WIDTHS) for r in (1, 2, 3)]

# Blend: geometry 0 (37 x 53, t = 16: tiles overlap, W % 4 != 0, the byte store) and geometry 5 (one 16 x 16 tile: the packed store) of
# tests/_segblend_cases.GEOMETRIES.  C = 9, 16, 17, 32 at both; the single tile also takes the exact fills 4 and 8 -- the ``C == CP``
# branch of seg_blend_predict_kernel, which the existing cases reach at 64 alone -- and 3, 5, 33, 64, so that every width runs both
# branches in this table.
BLEND_GEOMETRIES = (0, 5)
BLEND_KINDS = ("randn", "randn30")
BLEND_WINDOWS = ("gaussian", "constant")


def _blend(gi, C, k):
    F = (1, 4)[k % 2]
    return dict(kind="blend", name=f"{gi}-{C}", gi=gi, C=C, F=F, flips=[(2, 0, 3, 1)[(k + j) % 4] for j in range(F)], B=(1, 2)[(k // 2) % 2],
                window=BLEND_WINDOWS[(k + gi) % 2], logits=BLEND_KINDS[(k // 2 + gi) % 2], seed=2000 + 64 * gi + C,
                path=f"seg_blend_predict_kernel<{width(C)}>, C {'==' if C == width(C) else '<'} CP, {'one tile' if gi == 5 else 'overlapping tiles'}")


BLEND_CASES = [_blend(0, C, k) for k, C in enumerate((9, 16, 17, 32))] + [_blend(5, C, k) for k, C in enumerate((9, 16, 17, 32, 4, 8, 3, 5, 33, 64))]

CASES = LOSS_CASES + ACCESS_CASES + REFINE_CASES + BLEND_CASES
BY_NAME = {(c["kind"], c["name"]): c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ------------------------------------------------------------------------------------------ paths
def blend_geometry(gi: int):
    """(H, W, t, g, overlap) of tests/_segblend_cases.GEOMETRIES[gi], restated so that this module imports nothing."""
    return {0: (37, 53, 16, 4, 0.5), 5: (16, 16, 16, 4, 0.5)}[gi]


def reached(case: dict) -> set:
    """The compiled paths the mirror says ``case`` runs."""
    out = set()
    if case["kind"] == "loss":
        g, u, B, C = case["g"], case["u"], case["B"], case["C"]
        out |= {(k, width(C)) for k in LOSS_KERNELS}
        # a marker from the table's own CLASS_ENDS, not from the dispatch: it says which class counts the issue asks for at g = 3, B = 2,
        # and makes each class case needed by construction (the test beside it asserts their widths, g and B)
        if g == 3 and B == 2 and C in CLASS_ENDS:
            out.add(("class count", C))
        if g == 3 and u in FACTOR_WIDTHS:
            out |= {("cell", u, cw, R, "dead lanes" if 64 % cw else "no dead lane") for cw, R in cell_widths(g, u)}
        if g < 3 and u in (8, 32):
            out.add(("no interior cell", g, u))
    elif case["kind"] == "access":
        u = case["u"]
        out.add(("label load", u, "wide" if wide(case["yoff"], u) else "byte"))
        out.add(("prediction store", u, "wide" if wide(case["poff"], u) else "byte"))
    elif case["kind"] == "refine":
        out.add(("seg_refine_init", width(case["C"])))
        out.add(("seg_refine_iter", width(case["C"]), case["params"]["r"]))
    elif case["kind"] == "blend":
        H, W, t, g, _ = blend_geometry(case["gi"])
        out.add(("seg_blend_predict", width(case["C"]), "C == CP" if case["C"] == width(case["C"]) else "C < CP",
                 "one tile" if (H, W) == (t, t) else "overlapping tiles", "packed store" if W % 4 == 0 else "byte store"))
    return out


def full_set() -> set:
    """Every path the table has to reach."""
    full = {(k, cp) for k in LOSS_KERNELS for cp in WIDTHS}                      # every kernel x every CP, BD on and off
    full |= {("class count", C) for C in CLASS_ENDS}
    full |= {("cell", u, cw, 64 // cw, "dead lanes" if 64 % cw else "no dead lane") for u, ws in FACTOR_WIDTHS.items() for cw in ws}
    full |= {("no interior cell", g, u) for g in (1, 2) for u in (8, 32)}
    full |= {(what, u, how) for what in ("label load", "prediction store") for u in ACCESS_FACTORS for how in ("wide", "byte")}
    full |= {("seg_refine_init", cp) for cp in WIDTHS}
    full |= {("seg_refine_iter", cp, r) for cp in WIDTHS for r in (1, 2, 3)}
    full |= {("seg_blend_predict", cp, fill, "one tile", "packed store") for cp in WIDTHS for fill in ("C == CP", "C < CP")}
    full |= {("seg_blend_predict", cp, fill, "overlapping tiles", "byte store") for cp in (16, 32) for fill in ("C == CP", "C < CP")}
    return full


def reached_by(cases) -> set:
    out = set()
    for c in cases:
        out |= reached(c)
    return out
