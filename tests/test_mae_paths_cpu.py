"""The MAE path-complete tests without a device: the fp32 emulation of csrc/mae.hip (tests/_mae_emul.py) stays inside every a-priori
bound of tests/_mae_oracle.py at every shape tests/test_mae_paths_gpu.py runs; each of the nine planted defects leaves a bound or an
exact comparison in a named case; the three recorded cases of tests/golden/mae_parts.npz give the SAME bits with defects 1, 2, 3, 7 and 9
as without (so the suite before this module could not see them); no bound is looser than the 1e-5 it replaces; and the host-side
refusals tests/test_mae_cpu.py did not cover."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden

import _mae_emul as EM
import _mae_oracle as MO

RATIOS = {}


def ratio(name, got, ref, bound):
    """max error / bound; an element whose bound is 0 must be matched exactly, and a NaN (unwritten) element is infinitely wrong."""
    got, ref, bound = (np.asarray(a, np.float64) for a in (got, ref, bound))
    bound = np.broadcast_to(bound, ref.shape)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / bound)
    q = np.where(np.isnan(q), np.inf, q)
    out = float(q.max()) if q.size else 0.0
    if np.isfinite(out):
        RATIOS[name] = max(RATIOS.get(name, 0.0), out)
    return out


def exact(got, want):
    return bool(np.array_equal(np.asarray(got, np.float64), np.asarray(want, np.float64)))


_CASES = {}


def case(*key):
    if key not in _CASES:
        _CASES[key] = MO.make_case(*key)
    return _CASES[key]


# ------------------------------------------------------------------------------------------ judges: -> names of the checks that fail
def judge_mask(noise, Lk, defect=None):
    want_r, want_k = MO.mask_ids(noise, Lk)
    got_r, got_k = EM.mask_ids(noise, Lk, defect)
    bad = []
    if not (np.array_equal(got_r, want_r) and np.array_equal(got_k, want_k)):
        bad.append("mask_ids")
    if not all(np.array_equal(np.sort(r), np.arange(len(r))) for r in got_r):
        bad.append("mask_ids.permutation")
    return bad


def judge_unfold(c, ld=None, bf16=False, aligned=True, defect=None):
    V, H, W, p, L, Lk, D, K = c["dims"]
    ld = ld or K
    want = MO.gather_unfold(c["imgs"], c["ids_keep"], p, ld).astype(np.float32)
    want = MO.bf16_round(want) if bf16 else want
    return [] if exact(EM.gather_unfold(c["imgs"], c["ids_keep"], p, ld, bf16, defect, aligned), want) else ["gather_unfold"]


def judge_tokens(c, bf16=False, aligned=True, defect=None):
    V, H, W, p, L, Lk, D, K = c["dims"]
    patches = MO.bf16_round(c["patches"]) if bf16 else c["patches"]
    bad = []
    if not exact(EM.tokens_fwd(patches, c["cls"], c["pos"], c["ids_keep"], aligned, defect),
                 MO.tokens_fwd(patches, c["cls"], c["pos"], c["ids_keep"]).astype(np.float32)):
        bad.append("tokens_fwd")
    dp, dcls, dpos = EM.tokens_bwd(c["gtok"], c["ids_restore"], Lk, bf16, aligned, defect)
    o_dp, o_dcls, o_dpos = MO.tokens_bwd(c["gtok"], c["ids_restore"], Lk)
    want_dp = o_dp.astype(np.float32)
    if not exact(dp, MO.bf16_round(want_dp) if bf16 else want_dp):
        bad.append("dpatches")
    b = MO.bound_dpos(c["gtok"], c["ids_restore"], Lk)
    if ratio("dpos", dpos, o_dpos, b) > 1 or not np.array_equal(dcls, dpos[0], equal_nan=True):
        bad.append("dpos")
    if ratio("dcls", dcls, o_dcls, b[0]) > 1:
        bad.append("dcls")
    return bad


def judge_unshuffle(c, bf16=False, aligned=True, defect=None):
    V, H, W, p, L, Lk, D, K = c["dims"]
    e = MO.bf16_round(c["e"]) if bf16 else c["e"]
    bad = []
    if not exact(EM.unshuffle_fwd(e, c["mask_token"], c["dec_pos"], c["ids_restore"], aligned, defect),
                 MO.unshuffle_fwd(e, c["mask_token"], c["dec_pos"], c["ids_restore"]).astype(np.float32)):
        bad.append("unshuffle_fwd")
    de, dmask, _ = EM.unshuffle_bwd(c["gxd"], c["ids_keep"], c["ids_restore"], bf16, aligned, defect)
    o_de, o_dm = MO.unshuffle_bwd(c["gxd"], c["ids_keep"], c["ids_restore"])
    want_de = o_de.astype(np.float32)
    if not exact(de, MO.bf16_round(want_de) if bf16 else want_de):
        bad.append("de")
    if ratio("dmask_token", dmask, o_dm, MO.bound_dmask(c["gxd"], c["ids_restore"], Lk)) > 1:
        bad.append("dmask_token")
    return bad


def judge_loss(c, lead=0, bf16=False, aligned=True, defect=None):
    V, H, W, p, L, Lk, D, K = c["dims"]
    pred = MO.bf16_round(c["pred"]) if bf16 else c["pred"]
    full = np.concatenate([np.full((V, lead, K), 3.0, np.float32), pred], axis=1)
    vw = MO.loss_vw(p, aligned)
    loss, rows = EM.loss_fwd(full, c["imgs"], c["ids_restore"], Lk, p, lead, aligned, defect)
    o_rows = MO.loss_rows(pred, c["imgs"], c["ids_restore"], Lk, p)
    o_loss = MO.loss_fwd(pred, c["imgs"], c["ids_restore"], Lk, p)
    bad = []
    if ratio("row_loss", rows, o_rows, MO.bound_row_loss(o_rows, p, vw)) > 1:
        bad.append("row_loss")
    if ratio("loss", loss, o_loss, MO.bound_loss(o_loss, p, vw, V * L)) > 1:
        bad.append("loss")
    for gs in (1.0, 0.5):
        d = EM.loss_bwd(full, c["imgs"], c["ids_restore"], Lk, p, lead, gs, False, aligned, defect)
        o_d = MO.loss_bwd(pred, c["imgs"], c["ids_restore"], Lk, p, gs)
        if not exact(d[:, :lead], np.zeros((V, lead, K))) or ratio("dpred", d[:, lead:], o_d, MO.bound_dpred(o_d)) > 1:
            bad.append("dpred")
    return sorted(set(bad))


# ------------------------------------------------------------------------------------------ the emulation is inside every bound
@pytest.mark.parametrize("L", MO.MASK_L)
def test_emulated_mask_ids_equal_the_stable_argsort(L):
    for fam in MO.NOISE_FAMILIES:
        noise = MO.noise_family(fam, 3, L)
        for Lk in MO.mask_lks(L):
            if Lk < L:
                assert judge_mask(noise, Lk) == [], (fam, L, Lk)


@pytest.mark.parametrize("H,W,p", MO.UNFOLD_HWP)
def test_emulated_gather_unfold_is_exact(H, W, p):
    c = case(2, H, W, p, max((H // p) * (W // p) // 4, 1), 8, 1)
    K = 3 * p * p
    for bf16 in (False, True):
        for ld, aligned in ((K, True), (K + 16, True), (K, False)) + (((50, True),) if p == 4 else ()):
            assert judge_unfold(c, ld, bf16, aligned) == [], (ld, bf16, aligned)


@pytest.mark.parametrize("D", MO.TOKEN_D)
@pytest.mark.parametrize("L,Lk", MO.TOKEN_LLK)
def test_emulated_token_kernels_stay_inside_their_bounds(L, Lk, D):
    for V in MO.TOKEN_V:
        c = case(V, 1, L, 1, Lk, D, 2)
        for bf16 in (False, True):
            assert judge_tokens(c, bf16) == [] and judge_unshuffle(c, bf16) == [], (V, bf16)
        if D == 8:
            assert judge_tokens(c, aligned=False) == [] and judge_unshuffle(c, aligned=False) == []
        n, _ = MO.tokens_bwd_terms(c["gtok"], c["ids_restore"], Lk)
        dpos = EM.tokens_bwd(c["gtok"], c["ids_restore"], Lk)[2]
        assert not dpos[n == 0].any()                                          # positions nobody keeps: exactly 0


@pytest.mark.parametrize("H,W,p", MO.LOSS_HWP + [MO.LOSS_MEAN_HWP])
def test_emulated_loss_kernels_stay_inside_their_bounds(H, W, p):
    L = (H // p) * (W // p)
    c = case(3, H, W, p, max(L // 4, 1), 8, 3)
    for lead in (0, 1):
        for bf16 in (False, True):
            assert judge_loss(c, lead, bf16) == [], (lead, bf16)
    if p == 16:
        assert judge_loss(c, 0, False, aligned=False) == []                    # scalar, three trips


def test_emulated_grid_stride_second_trip():
    c = case(*MO.STRIDE_TOKENS)
    assert judge_tokens(c) == [] and judge_unshuffle(c) == []
    assert judge_unfold(case(*MO.STRIDE_UNFOLD), bf16=True) == []


def test_zz_print_emulation_ratios():
    for name, r in sorted(RATIOS.items()):
        print(f"ratio {name} {r:.3f}")
    assert RATIOS and max(RATIOS.values()) <= 1.0


# ------------------------------------------------------------------------------------------ planted defects
def test_every_planted_defect_is_flagged_in_a_named_case():
    flagged = {}
    rect = case(2, 8, 12, 4, 2, 8, 1)
    flagged[1] = judge_unfold(rect, defect=1) + judge_loss(case(3, 21, 35, 7, 3, 8, 3), defect=1)
    assert "gather_unfold" in flagged[1] and "row_loss" in flagged[1] and "dpred" in flagged[1]
    flagged[2] = judge_loss(case(3, 64, 96, 32, 1, 8, 3), defect=2) + judge_loss(case(3, 30, 45, 15, 1, 8, 3), defect=2)
    assert flagged[2].count("row_loss") == 2 and flagged[2].count("dpred") == 2 and "loss" in flagged[2]
    for D in (258, 1028):
        c = case(5, 1, 257, 1, 64, D, 2)
        flagged[3] = judge_tokens(c, defect=3) + judge_unshuffle(c, defect=3)
        assert "dpos" in flagged[3] and "dmask_token" in flagged[3], D
    flagged[4] = judge_loss(case(3, 28, 42, 14, 1, 8, 3), lead=1, defect=4)
    assert "row_loss" in flagged[4] and "dpred" in flagged[4]
    assert judge_loss(case(3, 28, 42, 14, 1, 8, 3), lead=0, defect=4) == []                       # (only lead = 1 can see it)
    flagged[5] = judge_mask(MO.noise_family("levels8", 3, 257), 64, defect=5)
    assert flagged[5] == ["mask_ids"] and judge_mask(MO.noise_family("equal", 3, 2), 1, defect=5) == ["mask_ids"]
    assert judge_mask(MO.noise_family("distinct", 3, 257), 64, defect=5) == []                    # (distinct noise cannot see it)
    flagged[6] = judge_mask(MO.noise_family("specials", 3, 255), 63, defect=6)
    assert flagged[6] == ["mask_ids"]
    c = case(*MO.STRIDE_TOKENS)
    flagged[7] = judge_tokens(c, defect=7) + judge_unshuffle(c, defect=7) + judge_unfold(case(*MO.STRIDE_UNFOLD), bf16=True, defect=7)
    assert flagged[7] == ["tokens_fwd", "dpatches", "unshuffle_fwd", "de", "gather_unfold"]
    flagged[8] = judge_loss(case(3, 21, 35, 7, 3, 8, 3), defect=8)
    assert flagged[8] == ["dpred"]
    for D in (1, 6, 258):
        c = case(1, 1, 2, 1, 1, D, 2)
        flagged[9] = judge_tokens(c, defect=9) + judge_unshuffle(c, defect=9)
        assert flagged[9] == ["tokens_fwd", "dpatches", "dpos", "dcls", "unshuffle_fwd", "de", "dmask_token"], D
    c = case(5, 1, 257, 1, 64, 8, 2)
    assert judge_tokens(c, aligned=False, defect=9) == [] and judge_tokens(c, defect=9) == []       # (D % 4 == 0 cannot see it)
    for n, text in EM.DEFECTS.items():
        print(f"defect {n} ({text}): flags {sorted(set(flagged[n]))}")
        assert flagged[n]


def _nan_equal(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


@pytest.mark.parametrize("tag", ["s16", "s196", "p14"])
def test_recorded_cases_cannot_see_defects_1_2_3_7_and_9(tag):
    """On the three cases of mae_parts.npz (square images, 3 p^2 <= 588, D <= 40, a few thousand work items, D % 4 == 0) the emulation
    gives the same bits with each of these defects as without, kernel by kernel: whatever a test asserts on those cases, it passes."""
    gold = load_golden("mae_parts.npz")
    V, L, Lk, D, p = (int(v) for v in gold[f"{tag}_dims"])
    ids_restore, ids_keep = MO.mask_ids(gold[f"{tag}_noise"], Lk)
    imgs, pred = gold[f"{tag}_imgs"], gold[f"{tag}_pred"]
    assert imgs.shape[2] == imgs.shape[3] and 3 * p * p <= 4 * MO.THREADS and D % 4 == 0 and D // 4 <= MO.THREADS
    assert V * (1 + L) * max(D, 3 * p * p) // 4 < EM.CAP
    kept = np.take_along_axis(gold[f"{tag}_patches"], ids_keep.astype(np.int64)[:, :, None], axis=1)
    g_full = np.random.default_rng(5).standard_normal((V, 1 + L, D)).astype(np.float32)

    def run(defect):
        out = [EM.gather_unfold(imgs, ids_keep, p, 3 * p * p, defect=defect)]
        out.append(EM.tokens_fwd(kept, gold[f"{tag}_cls"].reshape(-1), gold[f"{tag}_pos"][0], ids_keep, defect=defect))
        out += list(EM.tokens_bwd(gold[f"{tag}_gtok"], ids_restore, Lk, defect=defect))
        out.append(EM.unshuffle_fwd(gold[f"{tag}_e"], gold[f"{tag}_mask_token"].reshape(-1), gold[f"{tag}_dec_pos"][0], ids_restore, defect=defect))
        out += list(EM.unshuffle_bwd(g_full, ids_keep, ids_restore, defect=defect))
        out += list(EM.loss_fwd(pred, imgs, ids_restore, Lk, p, defect=defect))
        out.append(EM.loss_bwd(pred, imgs, ids_restore, Lk, p, defect=defect))
        return out
    clean = run(None)
    assert not any(np.isnan(np.asarray(a, np.float64)).any() for a in clean)
    for defect in (1, 2, 3, 7, 9):
        assert _nan_equal(run(defect), clean), defect
    assert not _nan_equal(run(8), clean)                                         # (a defect those cases do see)


# ------------------------------------------------------------------------------------------ no bound looser than the present 1e-5
def test_no_bound_is_looser_than_the_present_one():
    """Every bound is (constant) x (a magnitude no smaller than today's reference scale would be under the same test), so it is the
    constants that are compared: each is at most the 1e-5 tests/test_mae_gpu.py uses, at every shape of the device module."""
    worst = {}
    for V in MO.TOKEN_V + [MO.STRIDE_TOKENS[0]]:
        for L, Lk in MO.TOKEN_LLK + [(MO.STRIDE_TOKENS[2], MO.STRIDE_TOKENS[4])]:
            ids_restore, _ = MO.mask_ids(MO.noise_family("distinct", V, L), Lk)
            worst["dpos"] = max(worst.get("dpos", 0), MO.gamma(V - 1))
            worst["dmask_token"] = max(worst.get("dmask_token", 0), MO.dmask_constant(ids_restore, Lk))
            assert MO.dmask_constant(ids_restore, Lk) <= MO.gamma((L - Lk - 1) + (V - 1))       # never above the derived constant either
    for H, W, p in MO.LOSS_HWP + [MO.LOSS_MEAN_HWP]:
        for vw in {MO.loss_vw(p), 1}:
            worst["row_loss"] = max(worst.get("row_loss", 0), MO.gamma(MO.row_loss_roundings(p, vw)))
            worst["loss"] = max(worst.get("loss", 0), MO.gamma(MO.loss_roundings(p, vw, 3 * (H // p) * (W // p))))
    worst["dpred"] = MO.gamma(3)
    for k, v in sorted(worst.items()):
        print(f"constant {k} {v:.3e}")
        assert v <= MO.PRESENT_BAR, k
    assert MO.block_sum_depth() == 9 and MO.row_loss_roundings(32, 4) == 2 + 12 + 9 + 1 and MO.row_loss_roundings(7, 1) == 2 + 1 + 9 + 1


# ------------------------------------------------------------------------------------------ host-only refusals
def test_abi_refusals_missing_from_test_mae_cpu():
    """Fake pointers, never dereferenced: every one of these is DINOX_EINVAL before any launch, with its message."""
    from dinox import _lib
    lib = _lib.lib
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    E = -1
    # L = 17 x 241 = 4097 patches through the image entries
    assert lib.dinox_mae_gather_unfold(p, p, p, 2, 17, 241, 1, 4, 3, 0, None) == E and "L <= 4096" in _lib.last_error()
    assert lib.dinox_mae_loss_fwd(p, p, p, p, p, 2, 17, 241, 1, 4, 0, 0, None) == E and "L <= 4096" in _lib.last_error()
    assert lib.dinox_mae_loss_bwd(p, p, p, p + 128, 1.0, 2, 17, 241, 1, 4, 0, 0, 0, None) == E and "L <= 4096" in _lib.last_error()
    # patch = 33 > MAE_MAX_PATCH, both loss entries
    assert lib.dinox_mae_loss_fwd(p, p, p, p, p, 2, 66, 66, 33, 1, 0, 0, None) == E and "patch=33" in _lib.last_error() and "<= 32" in _lib.last_error()
    assert lib.dinox_mae_loss_bwd(p, p, p, p + 128, 1.0, 2, 66, 66, 33, 1, 0, 0, 0, None) == E and "patch=33" in _lib.last_error()
    # D = 65537
    for fn in (lib.dinox_mae_tokens_fwd, lib.dinox_mae_tokens_bwd, lib.dinox_mae_unshuffle_fwd):
        assert fn(p, p, p, p, p, 2, 16, 4, 65537, 0, None) == E and "D=65537" in _lib.last_error()
    assert lib.dinox_mae_unshuffle_bwd(p, p, p, p, p, p, 2, 16, 4, 65537, 0, None) == E and "D=65537" in _lib.last_error()
    # lead = 2 (the forward entry is in test_mae_cpu.py)
    assert lib.dinox_mae_loss_bwd(p, p, p, p + 128, 1.0, 2, 16, 16, 4, 4, 2, 0, 0, None) == E and "lead=2" in _lib.last_error()
    # H not a multiple of patch
    assert lib.dinox_mae_gather_unfold(p, p, p, 2, 15, 16, 4, 4, 48, 0, None) == E and "H=15" in _lib.last_error()
    assert lib.dinox_mae_loss_fwd(p, p, p, p, p, 2, 15, 16, 4, 4, 0, 0, None) == E and "multiples of patch" in _lib.last_error()
    assert lib.dinox_mae_loss_bwd(p, p, p, p + 128, 1.0, 2, 15, 16, 4, 4, 0, 0, 0, None) == E and "multiples of patch" in _lib.last_error()
