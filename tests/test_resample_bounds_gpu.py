"""csrc/views.hip and csrc/encode_prep.hip on the device, through the C ABI, element by element against the float64 statements and
a-priori bounds of oracle/resample_bounds.py (tests/test_resample_bounds_cpu.py holds an fp32 emulation to the same bounds on the same
cases and shows which planted defect each case flags).  Every operand sits in an allocation of its own between two guards of canary
bytes that must keep their bits (as tests/test_mae_paths_gpu.py does; its helpers are reused where the dtypes allow); every output
starts as NaN (or as a finite canary value where NaN is itself an expected result).  No element is excluded: the knife-edge indices
are covered by a term of the bound.  Every launch runs twice and must give the same bits.

Path -> the case that takes it:
  one tile / a last tile one pixel wide / 3 x 3 tiles with a last tile of 8      S = 16 / 17 / 40 of every family
  dynamic LDS above 64 KiB (reserve_lds)                                         lds64-16, mixed-16, mixed-17 (views); lds64-16-* (encode)
  the largest tables under the 150 KiB limit, and the refusal one pixel above    ldsmax-16 and test_*_refused_above_the_lds_limit
  the NaN tile (table too small for the crop / plane)                            test_understated_tables (C ABI only)
  nd outside 1..3; destination outside [0, 3 n_images)                           badnd-17-*, skipped-17-*
  a tiny crop beside the one that sizes the tables                               mixed-*
  the three output layouts of views.hip                                          test_views_patch_layouts"""
import numpy as np
import pytest
import torch

from oracle import resample_bounds as RB
from test_mae_paths_gpu import P, lib, ok, stream  # noqa: F401  (lib is the module fixture)

pytestmark = pytest.mark.gpu

DEV = "cuda"
PAD = 4096
CANARY_BYTE = 0xA5
NANF = np.float32(np.nan)
RATIOS = {}          # (kernel, stage, family) -> largest error / bound seen (printed by the last test; DESIGN.md "Resampling paths")


class Guarded:
    """Operands of one launch, any dtype: each in its own allocation with PAD canary bytes on both sides."""

    def __init__(self):
        self.all = []

    def put(self, name, arr):
        b = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        buf = torch.full((b.size + 2 * PAD,), CANARY_BYTE, dtype=torch.uint8, device=DEV)
        t = buf[PAD:PAD + b.size]
        t.copy_(torch.from_numpy(b.copy()))
        assert t.data_ptr() % 16 == 0
        self.all.append((name, buf, b.size))
        return t

    def fin(self):
        torch.cuda.synchronize()
        for name, buf, n in self.all:
            assert bool((buf[:PAD] == CANARY_BYTE).all()) and bool((buf[PAD + n:] == CANARY_BYTE).all()), f"canary of {name} moved"


def back(t, dtype, shape):
    return t.cpu().numpy().view(dtype).reshape(shape)


def note(kernel, stage, family, r):
    key = (kernel, stage, family)
    RATIOS[key] = max(RATIOS.get(key, 0.0), r)
    print(f"ratio {kernel} {stage} {family} {r:.3f}")


# ------------------------------------------------------------------------------------------ views
def run_views(lib, case, max_crop=None, patch=None, ld=None, bf16=False, expect=0):
    """-> (rc, the output as fp32 values, its raw bits)."""
    S, V = case["S"], len(case["views"])
    vi, vf = RB.view_tables(case["views"])
    g = Guarded()
    raw, dvi, dvf = g.put("raw", case["raw"]), g.put("view_i", vi), g.put("view_f", vf)
    mc = case["max_crop"] if max_crop is None else max_crop
    if patch is None:
        out = g.put("out", np.full((V, 3, S, S), NANF))
        rc = lib.dinox_slice_views(P(raw), P(dvi), P(dvf), P(out), V, S, mc, stream())
        shape, dt = (V, 3, S, S), np.float32
    else:
        rows = V * (S // patch) ** 2
        out = g.put("u", np.full((rows, ld), 0x7FC0, np.uint16) if bf16 else np.full((rows, ld), NANF))
        rc = lib.dinox_slice_views_patches(P(raw), P(dvi), P(dvf), P(out), V, S, mc, patch, ld, int(bf16), stream())
        shape, dt = (rows, ld), (np.uint16 if bf16 else np.float32)
    g.fin()
    assert rc == expect, (rc, expect)
    bits = back(out, dt, shape)
    vals = (bits.astype(np.uint32) << 16).view(np.float32) if dt == np.uint16 else bits
    return rc, vals, bits


@pytest.mark.parametrize("name", RB.VIEW_CASES)
def test_views_within_bounds(lib, name):
    case = RB.views_case(name)
    st = RB.statement(case)
    _, got, bits = run_views(lib, case)
    r = RB.judge(got, st)
    note("views", "image", case["family"], r)
    assert r <= 1.0, f"{name}: error / bound {r:.3f}"
    assert np.array_equal(bits.view(np.uint32), run_views(lib, case)[2].view(np.uint32))
    if case["family"] in ("lds64", "ldsmax"):
        assert RB.tables("views", case["S"], case["max_crop"])[2] > 64 * 1024
    if case["family"] == "ldsmax":
        assert RB.tables("views", case["S"], case["max_crop"] + 1)[2] > RB.LDS_LIMIT


def test_views_refused_above_the_lds_limit(lib):
    """One pixel more than the largest crop: DINOX_EUNSUPPORTED with its message, the NaN-filled output untouched."""
    import dinox._lib as L
    case = RB.views_case("ldsmax-16")
    _, got, _ = run_views(lib, case, max_crop=case["max_crop"] + 1, expect=-2)
    assert "LDS" in L.last_error() and "150 KiB" in L.last_error() and np.isnan(got).all()


@pytest.mark.parametrize("S,p,name", RB.PATCH_CASES)
def test_views_patch_layouts(lib, S, p, name):
    """The operand layouts: fp32 bit for bit the independent NumPy unfold of the image batch, bf16 bit for bit its RNE image, padded
    columns exact zeros; the image batch itself within its bounds."""
    case = RB.views_case(name)
    assert case["S"] == S and S % p == 0
    _, img, _ = run_views(lib, case)
    r = RB.judge(img, RB.statement(case))
    note("views", "image", "patch", r)
    assert r <= 1.0
    K = 3 * p * p
    for ld in (K, K + 24):
        want = RB.unfold(img, p, ld)
        _, u32, _ = run_views(lib, case, patch=p, ld=ld)
        assert np.array_equal(u32.view(np.uint32), want.view(np.uint32)), (p, ld)
        _, u16, b16 = run_views(lib, case, patch=p, ld=ld, bf16=True)
        assert np.array_equal(u16.view(np.uint32), RB.bf16_round(want).view(np.uint32)), (p, ld)
        assert not b16[:, K:].any() and not u32[:, K:].view(np.uint32).any()
        assert np.array_equal(b16, run_views(lib, case, patch=p, ld=ld, bf16=True)[2])
        note("views", "patches", f"p{p}", 0.0)


# ------------------------------------------------------------------------------------------ encode
def run_encode(lib, case, max_side=None, prefill=NANF, expect=0):
    S, n_img = case["S"], case["n_images"]
    g = Guarded()
    src, jobs = g.put("src", case["src"]), g.put("jobs", case["jobs"])
    out = g.put("out", np.full((n_img, 3, S, S), prefill, np.float32))
    lo, hi = case["level"] - case["width"] / 2, case["level"] + case["width"] / 2
    rc = lib.dinox_encode_preprocess(P(src), RB.DT_CODE[case["dtype"]], P(jobs), len(case["jobs"]), P(out), n_img, S,
                                     case["max_side"] if max_side is None else max_side, lo, hi, RB.FMT[case["fmt"]], stream())
    g.fin()
    assert rc == expect, (rc, expect)
    return back(out, np.float32, (n_img, 3, S, S))


@pytest.mark.parametrize("name", RB.ENC_CASES)
def test_encode_within_bounds(lib, name):
    case = RB.encode_case(name)
    st = RB.statement(case)
    got = run_encode(lib, case, prefill=RB.CANARY)
    r = RB.judge(got, st, prefill=RB.CANARY)
    note("encode", case["dtype"] + "/" + case["fmt"], case["family"], r)
    assert r <= 1.0, f"{name}: error / bound {r:.3f}"
    assert np.array_equal(got.view(np.uint32), run_encode(lib, case, prefill=RB.CANARY).view(np.uint32))
    if case["family"] == "planes":                                             # n == S stays the identity to the bit
        job = case["jobs"][-1]
        x, _ = RB.encode_window(RB.job_plane(case["src"], job), case["fmt"], case["level"] - case["width"] / 2, case["level"] + case["width"] / 2)
        want = ((x.astype(np.float32) - np.float32(0.406)) / np.float32(0.225)).astype(np.float32)
        assert int(job[6]) == 5 and np.array_equal(got[1, 2].view(np.uint32), want.view(np.uint32))
    if case["family"] in ("lds64", "ldsmax"):
        assert RB.tables("encode", case["S"], case["max_side"])[2] > 64 * 1024
    if case["family"] == "badnd":
        assert st["poisoned"].sum() == 7 and np.isnan(got.reshape(15, -1)[st["poisoned"]]).all()


def test_encode_refused_above_the_lds_limit(lib):
    import dinox._lib as L
    case = RB.encode_case("ldsmax-16-uint16-hu16_png")
    assert RB.tables("encode", 16, case["max_side"] + 1)[2] > RB.LDS_LIMIT
    got = run_encode(lib, case, max_side=case["max_side"] + 1, expect=-2)
    assert "LDS" in L.last_error() and "150 KiB" in L.last_error() and np.isnan(got).all()


# ------------------------------------------------------------------------------------------ tables stated too small (C ABI only)
@pytest.mark.parametrize("kind,name", [("views", "under-40"), ("encode", "under-40-float32-hu_float")])
def test_understated_tables(lib, kind, name):
    """max_crop / max_side stated as 80 where the launch holds 100: a refusal path, not a fault (a too-small table sets its tap count
    to -1 before any weight is written, a too-large footprint returns before any staging).  Every element NaN or within its bound, NaN in
    whole tiles, every tile whose footprint exceeds F by 2 or more is NaN, the guards intact."""
    case = RB.views_case(name) if kind == "views" else RB.encode_case(name)
    st = RB.statement(case)
    stated = case["max_crop"] if kind == "views" else case["max_side"]
    Fp, M, _ = RB.tables(kind, 40, stated)
    got = run_views(lib, case)[1] if kind == "views" else run_encode(lib, case)
    sides = [(v["h"], v["w"]) for v in case["views"]] if kind == "views" else [(100, 100)] * 2 + [(30, 44)]
    r = 0.0
    for v, (h, w) in enumerate(sides):
        must, mustnt = RB.tile_facts(kind, RB.axis(kind, w, 40), RB.axis(kind, h, 40), 40, Fp, M)
        assert must.any() or h <= stated
        for c in range(3) if kind == "views" else [0]:
            at = (v, c) if kind == "views" else (0, v)
            r = max(r, RB.judge_understated(got[at], {k: st[k][at] for k in ("ref", "bound")}, must, mustnt))
    note(kind, "understated", "under", r)


def test_zz_report_error_to_bound_ratios():
    for (kernel, stage, family), r in sorted(RATIOS.items()):
        print(f"max error / bound  {kernel:7s} {stage:26s} {family:10s} {r:.3f}")
    assert RATIOS and max(RATIOS.values()) <= 1.0
