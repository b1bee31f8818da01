"""oracle/resample_bounds.py on the CPU: the host-side table sizing checked exhaustively, the fp32 emulation of csrc/views.hip and
csrc/encode_prep.hip (tests/_resample_emul.py) inside the a-priori bounds on every case the device runs
(tests/test_resample_bounds_gpu.py), every planted defect flagged by a named case, and the host-side refusals of the two entry points.
No kernel is launched here."""
import json
import random

import numpy as np
import pytest

import _resample_emul as E
from conftest import load_golden
from oracle import resample_bounds as RB
from oracle import slice_views as SV

# defect -> the case that must flag it (and, for the patch layout, the operand shape)
FLAGGED_BY = {
    "flip_off_by_one": "corners-17", "flip_vertical_too": "corners-16", "taps_clipped_to_image": "corners-40", "sx_sy_swapped": "aspect-16",
    "support_from_other_axis": "aspect-17", "no_renormalisation": "slivers-40", "top_left_swapped": "corners-16",
    "plane_stride_from_crop": "corners-17", "wden_is_width": "window-16", "strip_without_fy0": "full-40", "patch_py_px_swapped": "patch-28",
    "enc_strides_swapped": "planes-17-float32-hu_float", "enc_channel0_normalisation": "planes-16-uint16-hu16_png",
    "enc_int16_as_uint16": "planes-40-int16-hu_float", "partial_tile_at_full_origin": "full-17",
}


# ------------------------------------------------------------------------------------------ table sizing
def test_tap_ranges_are_the_statements():
    for n, S in ((1, 16), (7, 17), (53, 17), (100, 16), (176, 40), (512, 224), (24, 40)):
        x0, xn = RB.views_tap_ranges(n, S)
        assert [(a, b) for a, b, _ in SV.aa_bicubic_weights(n, S)] == list(zip(x0.tolist(), xn.tolist()))
        x0, xn = RB.encode_tap_ranges(n, S)
        assert [(a, len(w)) for a, w in RB.pil_bilinear_weights(n, S)] == list(zip(x0.tolist(), xn.tolist()))


@pytest.mark.parametrize("kind", ["views", "encode"])
def test_table_sizing_exhaustive(kind):
    """F = int(16 s + 2 sup) + 4 and MAXT = int(2 sup) + 3, restated in oracle/resample_bounds.tables independently of the library: for
    every n in 1..2399 and every S of the list no tile footprint exceeds F, no tap count exceeds MAXT, no tap range is empty -- the NaN
    tile cannot be reached through make_views / device_preprocess, which size the tables from the largest side they hold."""
    worst_f, worst_t = 10 ** 9, 10 ** 9
    for S in RB.SIZING_S:
        for n in RB.SIZING_N:
            df, dt, least = RB.sizing_margins(kind, n, S)
            assert df >= 0 and dt >= 0 and least >= 1, (kind, n, S, df, dt, least)
            worst_f, worst_t = min(worst_f, df), min(worst_t, dt)
    print(f"{kind}: smallest F - footprint {worst_f}, smallest MAXT - taps {worst_t}")
    assert worst_f >= 3 and worst_t >= 2


def test_lds_formula_and_limit():
    assert RB.tables("views", 16, 100)[2] > 64 * 1024 and RB.tables("encode", 16, 110)[2] > 64 * 1024
    for kind in ("views", "encode"):
        n = RB.largest_side(kind, 16)
        assert RB.tables(kind, 16, n)[2] <= RB.LDS_LIMIT < RB.tables(kind, 16, n + 1)[2] and n + 1 <= 176


def test_library_lds_bytes_equal_the_restatement():
    from dinox._lib import lib
    for S, n in ((16, 100), (16, 144), (16, 145), (17, 53), (40, 176), (224, 1024), (16, 162), (16, 163)):
        assert lib.dinox_slice_views_lds_bytes(S, n) == RB.tables("views", S, n)[2]
        assert lib.dinox_encode_preprocess_lds_bytes(S, n) == RB.tables("encode", S, n)[2]


# ------------------------------------------------------------------------------------------ the emulation inside the bounds
@pytest.mark.parametrize("name", RB.VIEW_CASES)
def test_views_emulation_within_bounds(name):
    case = RB.views_case(name)
    st = RB.statement(case)
    r = RB.judge(E.views_emul(case), st)
    print(f"ratio views {name} {r:.3f}   held at the gate: {int(st['capped'].sum())} of {st['capped'].size}")
    assert r <= 1.0


@pytest.mark.parametrize("S,p,name", RB.PATCH_CASES)
def test_views_emulation_patch_layouts(S, p, name):
    case = RB.views_case(name)
    assert case["S"] == S
    img = E.views_emul(case)
    for ld in (3 * p * p, 3 * p * p + 24):
        u32 = E.views_emul(case, layout=2, p=p, ld=ld)
        assert np.array_equal(u32.view(np.uint32), RB.unfold(img, p, ld).view(np.uint32))
        u16 = E.views_emul(case, layout=1, p=p, ld=ld)
        assert np.array_equal(u16.view(np.uint32), RB.bf16_round(u32).view(np.uint32)) and not u16[:, 3 * p * p:].any()


@pytest.mark.parametrize("name", RB.ENC_CASES)
def test_encode_emulation_within_bounds(name):
    case = RB.encode_case(name)
    st = RB.statement(case)
    got = E.encode_emul(case, prefill=RB.CANARY)
    r = RB.judge(got, st, prefill=RB.CANARY)
    print(f"ratio encode {name} {r:.3f}   held at the gate: {int(st['capped'].sum())} of {st['capped'].size}")
    assert r <= 1.0
    if case["family"] == "planes":                                             # n == S is the identity to the bit
        job = case["jobs"][-1]
        x, _ = RB.encode_window(RB.job_plane(case["src"], job), case["fmt"], case["level"] - case["width"] / 2, case["level"] + case["width"] / 2)
        want = (x.astype(np.float32) - E.MEAN[2]) / E.STD[2]
        assert int(job[6]) == 5 and np.array_equal(got[1, 2].view(np.uint32), want.astype(np.float32).view(np.uint32))


def test_nan_cases_sit_away_from_a_knife_edge():
    """The tap ranges that hold the NaN are unambiguous: no tap in doubt is a row or column that holds one."""
    for name in (n for n in RB.ENC_CASES if n.startswith("nan")):
        case = RB.encode_case(name)
        job = case["jobs"][0]
        nan = np.isnan(RB.job_plane(case["src"], job).astype(np.float64))
        assert nan.sum() == 2
        for ax, hit in ((RB.axis("encode", int(job[2]), case["S"]), nan.any(0)), (RB.axis("encode", int(job[1]), case["S"]), nan.any(1))):
            d = ax["doubt"]
            assert not hit[d[d >= 0]].any()
        ref = RB.statement(case)["ref"]
        assert 0 < np.isnan(ref[0, 0]).sum() < ref[0, 0].size


@pytest.mark.parametrize("kind,name", [("views", "under-40"), ("encode", "under-40-float32-hu_float")])
def test_understated_tables_emulation(kind, name):
    """Tables sized for 80 where the launch holds 100 (possible through the C ABI alone): whole tiles of NaN, everything else in bounds."""
    case = RB.views_case(name) if kind == "views" else RB.encode_case(name)
    st = RB.statement(case)
    stated = case["max_crop"] if kind == "views" else case["max_side"]
    Fp, M, _ = RB.tables(kind, 40, stated)
    got = E.views_emul(case) if kind == "views" else E.encode_emul(case)
    sides = [(v["h"], v["w"]) for v in case["views"]] if kind == "views" else [(100, 100)] * 2 + [(30, 44)]
    n_nan = 0
    for v, (h, w) in enumerate(sides):
        must, mustnt = RB.tile_facts(kind, RB.axis(kind, w, 40), RB.axis(kind, h, 40), 40, Fp, M)
        for c in range(3) if kind == "views" else [0]:
            plane = (slice(v, v + 1), c) if kind == "views" else (slice(0, 1), v)
            RB.judge_understated(got[plane][0], {k: st[k][plane][0] for k in ("ref", "bound")}, must, mustnt)
        n_nan += int(must.sum())
        assert (h <= stated) == bool(mustnt.all())
    assert n_nan > 0


# ------------------------------------------------------------------------------------------ planted defects
def _run(name, defect):
    if name.split("-")[0] in ("planes",):
        case = RB.encode_case(name)
        return RB.flagged(E.encode_emul(case, defect=defect), RB.statement(case))
    case = RB.views_case(name)
    if defect == "patch_py_px_swapped":
        S, p = case["S"], 14
        st = RB.statement(case)
        want = {k: RB.unfold(st[k], p, 3 * p * p) for k in ("ref", "bound")}
        return RB.flagged(E.views_emul(case, layout=2, p=p, ld=3 * p * p, defect=defect), want)
    return RB.flagged(E.views_emul(case, defect=defect), RB.statement(case))


@pytest.mark.parametrize("defect", E.DEFECTS)
def test_planted_defect_is_flagged_by_its_named_case(defect):
    name = FLAGGED_BY[defect]
    assert not _run(name, None), f"{name} flags the emulation without a defect"
    assert _run(name, defect), f"{defect} passes {name}"


def _present_views():
    """The draws of two of the five batches of tests/test_slice_views.py::test_slice_views_vs_oracle (those with outputs of 32 and 40; the
    other three draw from the same distributions at 224) as cases of this module."""
    from dinox.views import draw_view
    out = []
    for shapes, size, crop_scale in (([(130, 70)], 32, (0.08, 1.0)), ([(200, 333)], 40, (0.5, 1.0))):
        seed = len(shapes) * 7 + size
        rng = np.random.default_rng(seed)
        random.seed(seed)
        views, parts, pos = [], [], 0
        for (H, W) in shapes:
            base = rng.integers(22768, 72768, size=(3, H // 4 + 1, W // 4 + 1)).astype(np.float32)
            img = np.kron(base, np.ones((1, 4, 4), dtype=np.float32))[:, :H, :W] + rng.normal(0, 300, (3, H, W))
            parts.append(np.clip(img, 0, 65535).astype(np.uint16).reshape(-1))
            for _ in range(2):
                p = draw_view(H, W, crop_scale=crop_scale)
                views.append(dict(off=pos, H=H, W=W, top=p.top, left=p.left, h=p.h, w=p.w, flip=p.flip, level=p.level, width=p.width))
            pos += 3 * H * W
        out.append(dict(kind="views", name=f"present-{size}", S=size, raw=np.concatenate(parts), views=views,
                        max_crop=max(max(v["h"], v["w"]) for v in views)))
    return out


def _present_encode():
    g = load_golden("encode_preprocess.npz")
    out = []
    for c in json.loads(str(g["cases"])):
        a = g[f"in_{c['name']}"]
        b = RB.EncodeBuilder(c["S"], f"golden-{c['name']}", "golden", str(a.dtype), c["format"], n_images=1, level=c["level"], width=c["width"])
        b.parts.append(np.ascontiguousarray(a).reshape(-1))
        if a.ndim == 2:
            b.job(0, a.shape[0], a.shape[1], a.shape[1], 1, [0, 1, 2])
        elif a.shape[2] == 3:
            for ch in range(3):
                b.job(ch, a.shape[0], a.shape[1], 3 * a.shape[1], 3, [ch])
        else:
            for ch in range(3):
                b.job(ch * a.shape[1] * a.shape[2], a.shape[1], a.shape[2], a.shape[2], 1, [ch])
        b.pos = a.size
        case = b.done()
        case["src"] = case["src"].astype(a.dtype)
        out.append((case, g[f"out_{c['name']}"]))
    return out


def present_cases_catch(defect) -> bool:
    """Would the cases the suite had before have flagged the defect at their flat 1e-5?"""
    if defect.startswith("enc_") or defect == "partial_tile_at_full_origin":
        for case, want in _present_encode():
            got = E.encode_emul(case, defect=defect)[0]
            if not (np.abs(got - want) <= 1e-5).all():
                return True
        if defect != "partial_tile_at_full_origin":
            return False
    if defect == "patch_py_px_swapped":
        return True                                    # test_slice_views_patches_is_unfold_of_slice_views compares with patch_unfold bit for bit
    for case in _present_views():
        got = E.views_emul(case, defect=defect)
        for v, p in enumerate(case["views"]):
            stack = case["raw"][p["off"]:p["off"] + 3 * p["H"] * p["W"]].reshape(3, p["H"], p["W"])
            want = SV.make_view(stack, p["level"], p["width"], p["top"], p["left"], p["h"], p["w"], p["flip"], case["S"])
            if not (np.abs(got[v] - want) <= 1e-5).all():
                return True
    return False


# what DESIGN.md "Resampling paths" records: the defects the earlier cases would NOT have flagged
MISSED_BEFORE = {"wden_is_width"}


def test_which_defects_the_earlier_cases_miss():
    for case, want in _present_encode():                                       # (the emulation itself passes them)
        assert (np.abs(E.encode_emul(case)[0] - want) <= 1e-5).all(), case["name"]
    missed = {d for d in E.DEFECTS if not present_cases_catch(d)}
    print("defects the earlier cases miss:", sorted(missed))
    assert missed == MISSED_BEFORE


# ------------------------------------------------------------------------------------------ host-side refusals
def test_host_side_refusals():
    """Arguments refused before any device call (every pointer is a non-null dummy that is never followed)."""
    from dinox._lib import last_error, lib
    P = 4096
    for f in (lib.dinox_slice_views_lds_bytes, lib.dinox_encode_preprocess_lds_bytes):
        assert f(0, 10) == -1 and f(16, 0) == -1 and f(-1, -1) == -1 and f(16, 16) > 0
    assert lib.dinox_slice_views(P, P, P, P, 65536, 16, 16, None) == -1 and "V=65536" in last_error()
    assert lib.dinox_slice_views(P, P, P, P, 0, 16, 16, None) == -1
    assert lib.dinox_slice_views(P, P, P, P, 1, 0, 16, None) == -1 and lib.dinox_slice_views(P, P, P, P, 1, 16, 0, None) == -1
    assert lib.dinox_slice_views(None, P, P, P, 1, 16, 16, None) == -1 and "null" in last_error()
    assert lib.dinox_slice_views_patches(P, P, P, P, 65536, 16, 16, 16, 768, 0, None) == -1
    assert lib.dinox_slice_views_patches(P, P, P, P, 1, 40, 16, 16, 768, 0, None) == -1 and "patch=16" in last_error()      # S % patch
    assert lib.dinox_slice_views_patches(P, P, P, P, 1, 32, 16, 16, 767, 0, None) == -1 and "ld=767" in last_error()        # ld < 3 p^2
    assert lib.dinox_slice_views_patches(P, P, P, P, 1, 32, 16, 0, 768, 0, None) == -1
    for bad in (2, 3, -1):
        assert lib.dinox_slice_views_patches(P, P, P, P, 1, 32, 16, 16, 768, bad, None) == -1 and "dtype" in last_error()
    enc = lambda **k: lib.dinox_encode_preprocess(*[{**dict(src=P, dt=0, jobs=P, n_jobs=1, out=P, n_images=1, S=16, max_side=16, lo=-160.0,
                                                            hi=240.0, fmt=0, stream=None), **k}[a]
                                                    for a in ("src", "dt", "jobs", "n_jobs", "out", "n_images", "S", "max_side", "lo", "hi", "fmt", "stream")])
    assert enc(n_jobs=65536) == -1 and "n_jobs=65536" in last_error()
    assert enc(n_jobs=0) == -1 and enc(n_images=0) == -1 and enc(S=0) == -1 and enc(max_side=0) == -1 and enc(src=None) == -1
    assert enc(S=16385, max_side=16385) == -1 and "S=16385" in last_error()
    for bad in (-1, 3):
        assert enc(fmt=bad) == -1 and "format" in last_error()
    for bad in (1, 4, -1):
        assert enc(dt=bad) == -1 and "source dtype" in last_error()
    # over the LDS limit: refused before the launch, with the message (the launches at and under the limit run in the GPU suite)
    assert lib.dinox_slice_views(P, P, P, P, 1, 16, RB.largest_side("views", 16) + 1, None) == -2 and "LDS" in last_error()
    assert enc(max_side=RB.largest_side("encode", 16) + 1) == -2 and "LDS" in last_error()
