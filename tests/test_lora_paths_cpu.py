"""The LoRA path table judged on the CPU (no kernel is launched here).

1. tests/_lora_paths_cases.py reaches every launch decision of csrc/lora.hip: the union of ``paths(...)`` over CASES is ALL_PATHS minus the
   tags documented as unreachable, and every tag names the case that covers it.
2. The bounds of tests/_lora_oracle.py are neither too tight nor vacuous on those cases: the kernels' stated arithmetic, evaluated in NumPy
   float32 in their order (LO.emulate_*), lies inside the bound on EVERY element of every case and value family, and where the chains are
   short (<= 64 terms, the condition of tests/test_gemm_contract_cpu.py) it uses more than 5e-3 of it; each planted defect (LO.MUTANTS) is
   flagged on the cases named in MUTANT_CASES.  An output that B = 0 fixes at an exact value is held to equality instead of a ratio:
   nothing is tighter, and an exact result cannot use a share of any bound.
"""
import numpy as np
import pytest

import _lora_oracle as LO
import _lora_paths_cases as LP


@pytest.fixture(scope="module")
def built():
    cache = {}

    def get(name, family):
        if (name, family) not in cache:
            c = LP.BY_NAME[name]
            o = LP.make(c, family)
            cache[(name, family)] = (c, o, LO.reference(c, o))
        return cache[(name, family)]
    return get


def out_sizes(c):
    M, K, N, r = c["M"], c["K"], c["N"], c["r"]
    return {"down": {"u": M * r}, "up": {"t": M * N}, "grad": {"dA": r * K, "dB": N * r}, "merge": {"out": N * K}}[c["entry"]]


def exact_outputs(c, o):
    """zeroB: the outputs that B = 0 (the small matrix, for down and up) fixes exactly, with their values."""
    e = c["entry"]
    if e == "down":
        return {"u": np.zeros((c["M"], c["r"]), np.float32)}
    if e == "up":
        return {"t": o["res"] if c["res"] != "none" else np.zeros((c["M"], c["N"]), np.float32)}
    if e == "grad":
        return {"dA": np.zeros((c["r"], c["K"]), np.float32)}
    return {"out": o["W"]}


# ------------------------------------------------------------------------------------------ 1. coverage
def test_cases_reach_every_reachable_path():
    cover = {}
    for c in LP.CASES:
        tags = LP.case_paths(c)
        assert tags <= LP.ALL_PATHS, (c["name"], sorted(tags - LP.ALL_PATHS))
        for t in tags:
            cover.setdefault(t, c["name"])
    for t in sorted(LP.ALL_PATHS):
        print(f"LORA-PATHS-CPU tag {t:34s} {cover.get(t) or 'UNREACHABLE: ' + LP.UNREACHABLE.get(t, '?')}")
    assert set(LP.UNREACHABLE) <= LP.ALL_PATHS and not set(LP.UNREACHABLE) & set(cover)
    missing = LP.ALL_PATHS - set(LP.UNREACHABLE) - set(cover)
    assert not missing, f"no case reaches {sorted(missing)}"
    assert len(LP.CASES) == len(LP.BY_NAME) <= 64
    for c in LP.CASES:                                  # a misaligned twin differs from its aligned case in `off` (and in place) alone
        if c["twin"]:
            t = LP.BY_NAME[c["twin"]]
            assert not t["off"] and c["off"] and all(c[k] == t[k] for k in ("entry", "M", "K", "N", "r", "dtype", "layout", "s", "sign"))


def test_every_flag_has_a_case_where_alignment_alone_decides():
    """Per entry and operand: a case with K % 4 == 0 (N % 4 == 0) and r % 4 == 0 whose only misaligned operand flips the flag."""
    want = {"down:vec:off:align", "down:svec:off:align", "up:VEC1:align:t", "up:VEC1:align:res", "up:VEC1:align:S", "up:r4:off:align:u",
            "up:r4:off:align:S", "grad:vecK:off:align", "grad:vecN:off:align", "grad:avec:off:align", "merge:VEC1:align:W", "merge:VEC1:align:out",
            "merge:VEC1:align:A"}
    seen = set()
    for c in LP.CASES:
        widths = {"down": ("K",), "up": ("N",), "grad": ("K", "N"), "merge": ("K",)}[c["entry"]]      # (merge's N counts rows)
        if c["twin"] and len(c["off"]) == 1 and c["r"] % 4 == 0 and all(c[w] % 4 == 0 for w in widths):
            seen |= LP.case_paths(c) - LP.case_paths(LP.BY_NAME[c["twin"]])
    assert want <= seen, sorted(want - seen)


# ------------------------------------------------------------------------------------------ 2. the emulation inside the bound
@pytest.mark.parametrize("name", [c["name"] for c in LP.CASES])
def test_emulation_lies_inside_the_bound_on_every_element(built, name):
    total = 0
    for family in LP.FAMILIES:
        c, o, ref = built(name, family)
        got = LO.emulate(c, o)
        exact = exact_outputs(c, o) if family == "zeroB" else {}
        assert set(got) == set(ref) == set(out_sizes(c))
        for k, (r64, bound) in ref.items():
            res = LO.check(got[k], r64, bound)
            total += res["compared"]
            print(f"LORA-PATHS-CPU {c['entry']} {name} {family} {k}: compared={res['compared']} ratio={res['ratio']:.3g} chain={LO.chain_length(c, k)}")
            assert res["compared"] == out_sizes(c)[k] == got[k].size, res              # every element, none exempt
            assert res["nan"] == 0 and res["canary"] == 0 and res["unwritten"] == 0, res
            assert res["ratio"] <= 1.0, (family, k, res)
            if k in exact:
                assert np.array_equal(got[k], exact[k]), (family, k)                      # exactly 0.0 (or the addend's other term), not small
            elif LO.chain_length(c, k) <= 64:
                assert res["ratio"] > 5e-3, f"the bound is vacuous on {name}/{family}/{k}: the emulated arithmetic uses {res['ratio']:.2e} of it"
    print(f"LORA-PATHS-CPU {name}: {total} elements compared = {len(LP.FAMILIES)} x {sum(out_sizes(LP.BY_NAME[name]).values())}")
    assert total == len(LP.FAMILIES) * sum(out_sizes(LP.BY_NAME[name]).values())


# which case shows which planted defect (randn values unless named otherwise)
MUTANT_CASES = {
    "ragged_tile_dropped": ["d-129x130-r33-bf16", "d-5x132-r8", "g-130x132x130-r40", "g-5x100x160-r8"],
    "up_remainder_dropped": ["u-5x36-r6-res", "u-257x130-r63-l1-res", "m-5x130-r33-neg-inplace"],
    "rank_ge32_dropped": ["d-129x130-r33-bf16", "d-130x132-r40-l1", "g-257x200x260-r63-bf16"],
    "rows_past_chunk_from_next": ["g-129x130x132-r33-bf16", "g-5x132x132-r8"],
    "last_chunk_left_out": ["g-130x132x130-r40", "g-129x130x132-r33-bf16"],
    "s_ignored": ["u-5x132-r8-res", "g-5x132x132-r8", "m-5x132-r8"],
    "s_per_chunk_and_end": ["g-129x130x132-r33-bf16", "g-5x132x132-r8"],
    "res_ignored": ["u-5x36-r6-res", "m-1x8-r1"],
    "clamped_row_past_M": ["u-5x36-r6-res", "u-129x130-r33-res"],
}


def test_mutant_table_is_complete():
    assert set(MUTANT_CASES) == set(LO.MUTANTS)
    for m, names in MUTANT_CASES.items():
        assert names and all(LP.BY_NAME[n]["entry"] in LO.MUTANTS[m] for n in names), m


@pytest.mark.parametrize("mutant,name", [(m, n) for m in MUTANT_CASES for n in MUTANT_CASES[m]])
def test_every_mutant_is_flagged(built, mutant, name):
    c, o, ref = built(name, "randn")
    got = LO.emulate(c, o, mutant)
    res = {k: LO.check(got[k], *ref[k]) for k in ref}
    worst = max(r["ratio"] for r in res.values())
    hits = sum(r["canary"] for r in res.values())
    print(f"LORA-PATHS-CPU mutant {mutant} on {name}: ratio={worst:.3g} canary={hits} -> flagged")
    assert worst > 1.0 or hits > 0 or any(r["nan"] for r in res.values()), f"{mutant} passes on {name}"
    if mutant == "clamped_row_past_M":
        assert hits == c["N"] and worst <= 1.0                   # one row of words in the guard, every value inside the bound


@pytest.mark.parametrize("entry", ["down", "up", "grad", "merge"])
def test_zero_B_outputs_of_the_emulation_are_exactly_zero(built, entry):
    n = 0
    for case in LP.CASES:
        if case["entry"] != entry:
            continue
        c, o, _ = built(case["name"], "zeroB")
        got = LO.emulate(c, o)
        if entry == "down":
            assert np.count_nonzero(got["u"]) == 0
        elif entry == "grad":
            assert np.count_nonzero(got["dA"]) == 0 and np.count_nonzero(got["dB"]) > 0
        else:                                                    # the addend: what the product adds to res / W
            k = "t" if entry == "up" else "out"
            base = o["W"] if entry == "merge" else (o["res"] if c["res"] != "none" else np.float32(0.0))
            assert np.count_nonzero(got[k] - base) == 0 and np.array_equal(got[k], np.broadcast_to(base, got[k].shape))
        n += 1
    assert n >= 8
