"""The exact-fp32 GEMM contract judged on the CPU (oracle/gemm_bounds.py, in_ = "f32" and the mixed layouts; tests/_colsum_emul.py).

1. The extension moved nothing: build() of every case the bf16 contract tests run gives the bytes it gave before Spec had `in_` and
   `trans_b` (tests/golden/gemm_bounds_build_digests.json, recorded from the module as it stood).
2. fma32 is an fma: it differs from the twice-rounded form on inputs built to double-round, and equals exact rational arithmetic.
3. The kernel's documented arithmetic -- one fma chain per output in ascending k -- is inside the unchanged bound on every element of
   every new family, uses a visible part of it at short K, and each planted defect (GB.F32_MUTANTS) is flagged on the families it
   applies to.
4. Host only: the dispatcher names gemm_f32 for every new case, and the mirror of launch_gemm_f32's tile predicate puts each case
   on the side of the line it was written for.
5. colsum_kernel's emulation: the case set covers its axes, its order is distinguishable from a plain ascending sum, it is inside
   its float64 bound, and the planted reassociation changes bits but stays inside that bound.
"""
import hashlib
import json
import os
from fractions import Fraction

import numpy as np
import pytest

import _colsum_emul as CS
import _gemm_raw as R
from oracle import gemm_bounds as GB

FAMILIES = dict(GB.f32_cpu_families())


# ------------------------------------------------------------------------------------------ 1. nothing that existed moved
def _existing_cases():
    for gen in (GB.strided_cases, GB.batched_cases, GB.alpha_cases):
        for k in GB.KERNELS:
            for n, s in gen(k):
                yield f"{gen.__name__}/{k}/{n}", s
    for n, (k, s, w) in GB.accum_cases():
        yield f"accum_cases/{n}", s
    for n, s in GB.misaligned_cases():
        yield f"misaligned_cases/{n}", s
    for n, s in GB.cpu_families():
        yield f"cpu_families/{n}", s


def _digest(bufs) -> str:
    h = hashlib.sha256()
    for name in sorted(bufs):
        b = bufs[name]
        h.update(f"{name}|{b.data.dtype.str}|{b.origin}|{b.data.size}|{b.idx.shape}|{int(b.output)}|".encode())
        h.update(b.data.tobytes())
        h.update(b.idx.astype("<i8").tobytes())
    return h.hexdigest()


def test_build_of_every_existing_case_is_byte_identical():
    with open(os.path.join(os.path.dirname(__file__), "golden", "gemm_bounds_build_digests.json")) as fh:
        want = json.load(fh)
    got = {k: _digest(GB.build(s)) for k, s in _existing_cases()}
    assert sorted(got) == sorted(want) and len(got) == 266
    moved = [k for k in want if got[k] != want[k]]
    assert not moved, moved
    for _, s in _existing_cases():
        assert s.in_ == "bf16" and s.trans_b is None and s.tb == s.trans


# ------------------------------------------------------------------------------------------ 2. the exact fma
def _round_fraction_f32(x: Fraction) -> np.float32:
    """x -> nearest float32, ties to even, in integers (normal range)."""
    if x == 0:
        return np.float32(0.0)
    sign, x = (-1, -x) if x < 0 else (1, x)
    e = x.numerator.bit_length() - x.denominator.bit_length() - 24
    while x >= Fraction(2) ** (e + 24):
        e += 1
    while x < Fraction(2) ** (e + 23):
        e -= 1
    y = x / Fraction(2) ** e                         # 2^23 <= y < 2^24
    q, r = divmod(y.numerator, y.denominator)
    twice = 2 * r
    if twice > y.denominator or (twice == y.denominator and q & 1):
        q += 1
    return np.float32(sign * float(q) * 2.0 ** e)       # q <= 2^24 and the scaling by 2^e are exact in float64


def _double_rounding_inputs():
    """(a, b, c): a b = +-(2^2n - 1), c a float32 one away from a float32 tie point: the exact sum is the tie -+ 1, float64 (ulp
    2^(2n - 28) there, n >= 15) rounds it ONTO the tie, and the tie then goes to the even neighbour -- the wrong one when j makes
    the right one odd."""
    for n in range(15, 24):
        for j in (1, 3, 5, 1001):
            for sc in (1.0, 2.0 ** -70, -(2.0 ** -41)):          # as built, in another binade, and with all signs mirrored
                # tie T = (2^24 + 2 j + 1) 2^2n.  c = T - 2^2n (odd mantissa), a b = 2^2n - 1: exact = T - 1, nearest is c
                yield float(2 ** n + 1) * sc, float(2 ** n - 1), float((2 ** 24 + 2 * j) * 2 ** (2 * n)) * sc
                # c = T + 2^2n (mantissa j + 1 with j + 1 odd below), a b = -(2^2n - 1): exact = T + 1, nearest is c
                yield -float(2 ** n + 1) * sc, float(2 ** n - 1), float((2 ** 24 + 2 * (j + 2)) * 2 ** (2 * n)) * sc


def test_fma32_rounds_once_where_float64_rounds_twice():
    tri = np.array(list(_double_rounding_inputs()), dtype=np.float64)
    assert (tri.astype(np.float32).astype(np.float64) == tri).all()                 # the inputs ARE float32 values
    a, b, c = (tri[:, i].astype(np.float32) for i in range(3))
    got, twice = GB.fma32(a, b, c), GB.fma32_double_rounded(a, b, c)
    want = np.array([_round_fraction_f32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a, b, c)])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert (twice != want).all(), "the constructed inputs do not double-round: the check above proves nothing"


def test_fma32_equals_rational_arithmetic():
    rng = np.random.default_rng(5)
    n = 600
    a = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 6, n)).astype(np.float32)
    b = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 6, n)).astype(np.float32)
    c = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 6, n)).astype(np.float32)
    near = np.arange(n) % 3 == 0                                                    # a third with c near -a b: cancellation
    c[near] = (-(a[near].astype(np.float64) * b[near].astype(np.float64)) * (1 + rng.standard_normal(near.sum()) * 1e-6)).astype(np.float32)
    got = GB.fma32(a, b, c)
    want = np.array([_round_fraction_f32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a, b, c)])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(GB.fma32(a.reshape(20, 30), b.reshape(20, 30), c[0]).reshape(-1).view(np.uint32),
                          GB.fma32(a, b, np.full(n, c[0], np.float32)).view(np.uint32))           # broadcasting, a scalar addend


# ------------------------------------------------------------------------------------------ 3. bound, emulation, planted defects
@pytest.fixture(scope="module")
def built():
    """name -> (spec, buffers, reference), computed once and left unchanged."""
    out = {}
    for name, s in FAMILIES.items():
        bufs = GB.build(s)
        out[name] = (s, bufs, GB.reference(s, bufs))
    return out


def _n_outputs(s, bufs):
    return sum(bufs[k].idx.size for k in GB.OUTPUTS if k in bufs and GB.is_output(s, k))


@pytest.mark.parametrize("name", list(FAMILIES))
def test_fma_chain_is_inside_the_bound(built, name):
    s, bufs, ref = built[name]
    r = GB.check(s, bufs, GB.emulate(s, bufs, "seq"), ref)
    print(f"GEMM-F32-CONTRACT-CPU {name}: " + " ".join(f"{k}={v:.3g}" for k, v in r.items() if k.startswith("ratio")))
    assert r["compared"] == _n_outputs(s, bufs) and r["exempt"] == 0
    assert r["ok"], r
    if s.K <= 64:
        assert r["ratio"] > 5e-3, f"the bound is vacuous on {name}: the emulated arithmetic uses {r['ratio']:.2e} of it"


def test_operands_are_stored_in_their_own_type_and_layout(built):
    for name, (s, bufs, _) in built.items():
        want = np.uint16 if s.in_ == "bf16" else np.float32
        assert bufs["A"].data.dtype == want and bufs["B"].data.dtype == want, name
        assert bufs["A"].idx.shape[1:] == ((s.K, s.M) if s.trans else (s.M, s.K)), name
        assert bufs["B"].idx.shape[1:] == ((s.K, s.N) if s.tb else (s.N, s.K)), name
        for k in ("A", "B"):
            pad = np.ones(bufs[k].data.shape, dtype=bool)
            pad[bufs[k].idx.reshape(-1)] = False
            v = GB.bf16_to_f64(bufs[k].data[pad]) if s.in_ == "bf16" else bufs[k].data[pad]
            assert np.isnan(v).all() and np.isfinite(bufs[k].live()).all() and pad[:GB.GUARD].all() and pad[-GB.GUARD:].all(), (name, k)


def test_overlapping_batch_items_share_no_element_and_leave_no_hole():
    for name, big, s in GB.f32_overlapped_stride_cases():
        bufs = GB.build(s)
        for k, rows in (("A", s.M), ("B", s.N)):
            b = bufs[k]
            kt = s.K * s.batch
            assert (s.lda, s.ldb, s.stride_a, s.stride_b) == (kt, kt, s.K, s.K)
            flat = np.sort(b.idx.reshape(-1))
            assert (np.diff(flat) == 1).all() and flat[0] == b.origin and flat.size == rows * kt, (name, k)     # one dense [rows][K_total]
            assert np.isnan(b.data[:b.origin]).all() and np.isnan(b.data[flat[-1] + 1:]).all() and np.isfinite(b.data[flat]).all()
        c = bufs["C"]
        pad = np.ones(c.data.shape, dtype=bool)
        pad[c.idx.reshape(-1)] = False
        assert (c.words()[pad] == GB.CANARY_F32).all() and pad.sum() >= 2 * GB.GUARD


# which family shows which planted defect (every mutant is tried on every family named here and must be flagged there)
_K44 = [n for n in FAMILIES if n.startswith("layout-77x24x44")]
F32_MUTANT_FAMILIES = {
    "odd_k_dropped": [n for n in FAMILIES if FAMILIES[n].K % 2],
    "stale_last_slab": [n for n in FAMILIES if FAMILIES[n].K > 16],
    "trans_b_follows_a": [n for n in FAMILIES if FAMILIES[n].tb != FAMILIES[n].trans],
    # (M = 33, 65, 129: the last block holds row 0 of the map alone, which the permutation leaves in place)
    "edge_row_map": _K44 + ["overlapped"] + [n for n in FAMILIES if n.startswith("colsum-")],
    "batch_stride_as_extent": ["big-own-b", "overlapped"],
}


def test_mutant_table_is_not_thin():
    assert set(F32_MUTANT_FAMILIES) == set(GB.F32_MUTANTS)
    assert len(F32_MUTANT_FAMILIES["odd_k_dropped"]) >= 8 and len(F32_MUTANT_FAMILIES["stale_last_slab"]) >= 12
    assert len(F32_MUTANT_FAMILIES["trans_b_follows_a"]) >= 8 and len(F32_MUTANT_FAMILIES["edge_row_map"]) >= 8


@pytest.mark.parametrize("mutant,name", [(m, f) for m in GB.F32_MUTANTS for f in F32_MUTANT_FAMILIES[m]])
def test_every_f32_mutant_is_flagged(built, mutant, name):
    s, bufs, ref = built[name]
    r = GB.check(s, bufs, GB.emulate(s, bufs, "seq", mutant), ref)
    print(f"GEMM-F32-CONTRACT-CPU mutant {mutant} on {name}: ratio={r['ratio']:.3g} nan={r['nan']} canary={r['canary']}")
    assert not r["ok"], f"{mutant} on {name} passes: {r}"
    assert r["canary"] == 0                              # these defects stay inside the tile: elements, never padding


# ------------------------------------------------------------------------------------------ 4. dispatcher and tile form, host only
def _all_new_cases():
    for n, s in GB.f32_layout_cases():
        yield "layout/" + n, s
    for n, s in GB.f32_k_edge_cases():
        yield "kedge/" + n, s
    for n, _, s in GB.f32_big_cases():
        yield "big/" + n, s
    for n, _, s in GB.f32_overlapped_stride_cases():
        yield "overlapped/" + n, s
    for n, s in GB.f32_colsum_cases():
        yield "colsum/" + n, s


def test_every_new_case_is_named_gemm_f32(monkeypatch):
    for k in ("DINOX_NT_PP", "DINOX_NT_PP384", "DINOX_NT_AREG_MAXK", "DINOX_FC1_AREG"):
        monkeypatch.delenv(k, raising=False)
    names = [n for n, _ in _all_new_cases()]
    assert len(names) == len(set(names)) and len(names) > 90
    for n, s in _all_new_cases():
        assert R.kernel_name(s) == "gemm_f32", n
        assert R.admits("gemm_f32", s, False)
        assert R.ws_bytes(s) == 0, n


def test_tile_form_mirror_agrees_with_what_each_case_is_for():
    for n, big, s in list(GB.f32_big_cases()) + list(GB.f32_overlapped_stride_cases()):
        assert GB.uses_big_tiles(s) == big, n
    for n, s in list(GB.f32_layout_cases()) + list(GB.f32_k_edge_cases()) + list(GB.f32_colsum_cases()):
        assert not GB.uses_big_tiles(s), n
    b = {n: s for n, _, s in GB.f32_big_cases()}
    on = b["129x130x37b64-00-f32-own_b"]
    assert -(-on.M // 128) * -(-on.N // 128) * on.batch == 256                       # exactly on the line
    assert GB.uses_big_tiles(on) and not GB.uses_big_tiles(on.but(batch=63)) and not GB.uses_big_tiles(on.but(M=127, batch=512))
    # the pieces that claim (a) launches fall on the 64-tile kernel
    for n, big, s in GB.f32_big_cases():
        if big:
            for sp, _, _ in R.pieces(s, "item" if s.batch > 1 else "strip"):
                assert not GB.uses_big_tiles(sp), n


def test_layout_cases_cover_what_they_promise():
    seen, epi_layouts, epi_outs = set(), {}, {}
    for n, s in GB.f32_layout_cases():
        seen.add((s.trans, s.tb, s.in_, s.out, (s.M, s.N, s.K)))
        name = n.rsplit("-", 1)[1]
        epi_layouts.setdefault(name, set()).add((s.trans, s.tb))
        epi_outs.setdefault(name, set()).add(s.out)
        assert s.lda > s.a_shape[1] and s.ldb > s.b_shape[1] and s.ldc > s.N and s.ldr > s.N and s.ldaux > s.N
        assert len({s.pad_a, s.pad_b, s.pad_c, s.pad_r, s.pad_x}) == 5
    assert len(seen) == 4 * 2 * 2 * 2
    assert set(epi_layouts) == set(GB.F32_EPILOGUES)
    for name in GB.F32_EPILOGUES:
        assert len(epi_layouts[name]) >= 2, name
        assert epi_outs[name] == ({"f32"} if name == "accum_bias" else {"f32", "bf16"}), name


# ------------------------------------------------------------------------------------------ 5. the column sum
def test_colsum_cases_cover_every_axis_value():
    cases = CS.cases()
    assert len(cases) <= 60 and len({c[0] for c in cases}) == len(cases)
    assert {(M, bf) for _, M, _, _, bf, _ in cases} == {(M, bf) for M in CS.MS for bf in (False, True)}
    assert {N for _, _, N, _, _, _ in cases} == set(CS.NS)
    assert {ld - N for _, _, N, ld, _, _ in cases} == {0, 3}
    assert {ac for *_, ac in cases} == {False, True}
    for N in CS.NS:                                                                  # every N with both pitches and both modes
        assert {(ld - N, ac) for _, _, n, ld, _, ac in cases if n == N} >= {(0, False), (3, True)} or \
               {(ld - N, ac) for _, _, n, ld, _, ac in cases if n == N} >= {(0, True), (3, False)}, N


def test_colsum_emulation_is_ordered_bounded_and_its_mutant_is_bits_only():
    differs = flat_differs = 0
    cases = CS.cases()
    for name, M, N, ld, bf, ac in cases:
        raw, live, out, out_in = CS.build(M, N, ld, bf, ac)
        assert np.isfinite(live).all() and live.shape == (M, N)
        pad = np.ones(raw.shape, dtype=bool)
        pad[CS.GUARD + np.arange(M).reshape(-1, 1) * ld + np.arange(N)] = False
        assert np.isnan(CS.bf16_to_f32(raw[pad]) if bf else raw[pad]).all()
        got = CS.colsum32(live, out_in)
        ref, bound = CS.reference(live, out_in)
        assert (np.abs(got.astype(np.float64) - ref) <= bound).all(), name
        differs += int((got.view(np.uint32) != CS.ascending32(live, out_in).view(np.uint32)).any())
        flat = CS.colsum32(live, out_in, "flat_join")
        assert (np.abs(flat.astype(np.float64) - ref) <= bound).all(), name
        flat_differs += int((flat.view(np.uint32) != got.view(np.uint32)).any())
    # M <= 16: one row per group, the tree against the chain; a single column of one or two rows cannot differ
    assert differs > 0.7 * len(cases), f"only {differs} of {len(cases)} cases tell the kernel's order from an ascending sum"
    assert flat_differs >= 10, flat_differs
    # the order itself, on a case small enough to write down: M = 3 -> groups 0, 1, 2 hold one row each, the tree adds (r0 + r1) + r2
    x = np.array([[1.0], [2.0 ** -24], [2.0 ** -24]], dtype=np.float32)
    assert CS.colsum32(x)[0] == np.float32(1.0) and CS.colsum32(x[::-1].copy())[0] == np.float32(1.0 + 2.0 ** -23)
    # M = 65, one group: rows 0, 16, 32, 48 go to s0..s3 and row 64 to s0 -- (x0 + x64) + x16 first
    x = np.zeros((65, 1), dtype=np.float32)
    x[0], x[16], x[64] = 1.0, 2.0 ** -24, 2.0 ** -24
    assert CS.colsum32(x)[0] == np.float32(1.0)                                     # (1 + 2^-24) -> 1, + 2^-24 -> 1
    x[0], x[16], x[64] = 2.0 ** -24, 1.0, 2.0 ** -24
    assert CS.colsum32(x)[0] == np.float32(1.0 + 2.0 ** -23)                        # (2^-24 + 2^-24) + 1


def test_splitk_bound_holds_for_the_documented_arithmetic_and_is_not_vacuous():
    rng = np.random.default_rng(9)
    M, N, kc, splits = 9, 7, 128, 8
    A = rng.standard_normal((M, kc * splits)).astype(np.float32)
    B = rng.standard_normal((N, kc * splits)).astype(np.float32)
    parts = np.zeros((splits, M, N), dtype=np.float32)
    for c in range(splits):
        for k in range(c * kc, (c + 1) * kc):
            parts[c] = GB.fma32(A[:, k, None], B[None, :, k], parts[c])
    got = CS.colsum32(parts.reshape(splits, M * N)).reshape(M, N)
    ref, bound = GB.splitk_reference(A.astype(np.float64), B.astype(np.float64), splits)
    ratio = np.abs(got - ref) / bound
    assert ratio.max() <= 1.0 and ratio.max() > 1e-3, ratio.max()
    parts[splits - 1] = 0                                                           # a chunk lost: far outside
    lost = CS.colsum32(parts.reshape(splits, M * N)).reshape(M, N)
    assert (np.abs(lost - ref) / bound).max() > 100
