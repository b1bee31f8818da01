"""Every path of csrc/mae.hip on the device, through the C ABI, against the float64 statements and a-priori bounds of
tests/_mae_oracle.py (tests/test_mae_paths_cpu.py holds an fp32 emulation to the same bounds and shows which planted defects each case
catches).  Every operand sits in its own allocation between two guards of 1024 canary elements that must keep their bits; every output
starts as NaN (ids: a sentinel) and must be written completely.

Launch predicate -> the case that takes it (all template instances of mae.hip):
  mae_mask_ids_kernel                 one trip L <= 256: L = 2, 255, 256; more: L = 257, 1369, 4096 (test_mask_ids)
  mae_gather_unfold_kernel<DT, 4>     p % 4 == 0, ld % 4 == 0, x and u aligned: p = 4, 16, 32, ld = 3 p^2 and 3 p^2 + 16, fp32 and bf16
  mae_gather_unfold_kernel<DT, 1>     p = 7, 14 (p % 4 != 0); p = 4 with ld = 50; x or u one element off; fp32 and bf16
  mae_tokens_fwd/bwd_kernel<DT, 4>    D = 8, 260, 1028 (1028: chunks = 2 in bwd), fp32 and bf16 patches
  mae_tokens_fwd/bwd_kernel<DT, 1>    D = 1, 6, 258 (258: chunks = 2); D = 8 with any one of patches / cls / pos / tokens (fwd), dtokens /
                                      dpatches / dcls / dpos (bwd) one element off
  mae_unshuffle_fwd/bwd_kernel<DT, 4|1>, mae_colsum_rows_kernel<4|1>      the same D and dtypes; e / mask_token / dec_pos / xd, g / de /
                                      dmask_token / ws one element off
  mae_loss_rows_kernel<DT, 4>         p = 14, 16, 18, 32 (K = 588, 768, 972, 3072: 1, 1, 1, 3 trips), fp32 and bf16 pred, lead 0 and 1
  mae_loss_rows_kernel<DT, 1>         p = 7, 15 (K = 147, 675: 1 and 3 trips); p = 16 with pred one element off (3 trips)
  mae_loss_bwd_kernel<DT, DTO, 4|1>   the four dtype pairs at p = 16 (vector) and at p = 7 (scalar); dpred one element off
  mae_loss_mean_kernel                V L = 18 .. 72 rows (one trip) and 1200 rows (five trips): H = W = 80, p = 4
  grid_1d cap, second trip            test_grid_stride_second_trip: every looping kernel with just over 4096 * 256 work items
  H != W                              every image case; L = 257, 300 token cases are 1 x L images of 1 x 1 patches"""
import numpy as np
import pytest
import torch

import _mae_oracle as MO

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 1024
SENTINEL = -7777
IVIEW = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.int32: torch.int32}
CANARY = {torch.float32: 0x7fc0dead, torch.bfloat16: 0x7fcd, torch.int32: 0x7fc0dead}
F32, BF16, I32 = torch.float32, torch.bfloat16, torch.int32
RATIOS = {}          # kernel output -> largest error / bound seen (printed by the last test; DESIGN.md "MAE paths" records them)


@pytest.fixture(scope="module")
def lib():
    import dinox._lib as L
    assert L.lib.dinox_device_ok() == 1, L.last_error()
    return L.lib


def stream():
    return torch.cuda.current_stream().cuda_stream


def ok(rc):
    import dinox._lib as L
    assert rc == 0, L.last_error()


class Operands:
    """The operands of one launch: each in an allocation of its own, GUARD canary elements on both sides; ``off`` names the one operand
    that starts one element past a 16-byte boundary (the ``off1`` of tests/test_sinkhorn_gpu.py)."""

    def __init__(self, off=None):
        self.off, self.hit, self.all, self.outs = off, False, [], []

    def _alloc(self, name, shape, dtype):
        n = int(np.prod(shape))
        o = 1 if name == self.off else 0
        buf = torch.empty(n + 2 * GUARD + 8, dtype=dtype, device=DEV)
        bits = buf.view(IVIEW[dtype])
        bits.fill_(CANARY[dtype])
        t = buf[GUARD + o:GUARD + o + n].view(tuple(shape))
        assert (t.data_ptr() % 16 != 0) if o else (t.data_ptr() % 16 == 0)
        self.hit |= bool(o)
        self.all.append((name, bits, GUARD + o, GUARD + o + n, CANARY[dtype]))
        return t

    def inp(self, name, a, dtype=F32):
        a = torch.from_numpy(np.ascontiguousarray(a))
        t = self._alloc(name, a.shape, dtype)
        t.copy_(a.to(dtype))
        return t

    def out(self, name, shape, dtype=F32):
        t = self._alloc(name, shape, dtype)
        t.fill_(SENTINEL if dtype == I32 else float("nan"))
        self.outs.append((name, t))
        return t

    def fin(self):
        """After the launches: every canary keeps its bits, every output element was written."""
        torch.cuda.synchronize()
        assert self.off is None or self.hit, self.off
        for name, bits, lo, hi, can in self.all:
            assert bool((bits[:lo] == can).all()) and bool((bits[hi:] == can).all()), f"canary of {name} moved"
        for name, t in self.outs:
            assert not bool((t == SENTINEL).any() if t.dtype == I32 else torch.isnan(t).any()), f"{name} has unwritten elements"


def P(t):
    return t.data_ptr()


def npf(t):
    return t.detach().float().cpu().numpy()


def within(name, got, ref, bound):
    """error <= bound elementwise; where the bound is 0 the value is exact."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    bound = np.broadcast_to(np.asarray(bound, np.float64), ref.shape)
    assert got.shape == ref.shape and np.isfinite(got).all(), name
    err = np.abs(got - ref)
    assert (err[bound == 0] == 0).all(), f"{name}: an element that must be exact is not"
    r = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    RATIOS[name] = max(RATIOS.get(name, 0.0), r)
    print(f"ratio {name} {r:.3f}")
    assert r <= 1.0, f"{name}: error / bound = {r:.3f}"


_CASES, _ORACLE = {}, {}


def case(*key):
    if key not in _CASES:
        _CASES[key] = MO.make_case(*key)
    return _CASES[key]


def oracle(key, fn):
    """float64 results computed once per (case, quantity) and shared."""
    if key not in _ORACLE:
        _ORACLE[key] = fn()
    return _ORACLE[key]


def bf(a, bf16):
    return MO.bf16_round(a) if bf16 else np.asarray(a, np.float32)


# ------------------------------------------------------------------------------------------ mask_ids
def run_mask_ids(lib, noise, Lk):
    V, L = noise.shape
    o = Operands()
    n, r, k = o.inp("noise", noise), o.out("ids_restore", (V, L), I32), o.out("ids_keep", (V, Lk), I32)
    ok(lib.dinox_mae_mask_ids(P(n), P(r), P(k), V, L, Lk, stream()))
    o.fin()
    return r.cpu().numpy(), k.cpu().numpy()


@pytest.mark.parametrize("fam", MO.NOISE_FAMILIES)
@pytest.mark.parametrize("L", MO.MASK_L)
def test_mask_ids(lib, L, fam):
    noise = MO.noise_family(fam, 3, L)
    for Lk in MO.mask_lks(L):
        if Lk >= L:
            continue
        want_r, want_k = oracle(("mask", fam, L, Lk), lambda: MO.mask_ids(noise, Lk))
        r, k = run_mask_ids(lib, noise, Lk)
        assert np.array_equal(r, want_r) and np.array_equal(k, want_k), (fam, L, Lk)
        assert all(np.array_equal(np.sort(row), np.arange(L)) for row in r)
        r2, k2 = run_mask_ids(lib, noise, Lk)
        assert np.array_equal(r, r2) and np.array_equal(k, k2)


# ------------------------------------------------------------------------------------------ gather_unfold
def run_gather_unfold(lib, c, ld, bf16, off=None, ids_keep=None):
    V, H, W, p, L, Lk, D, K = c["dims"]
    o = Operands(off)
    x, ids = o.inp("x", c["imgs"]), o.inp("ids_keep", c["ids_keep"] if ids_keep is None else ids_keep, I32)
    u = o.out("u", (V * Lk, ld), BF16 if bf16 else F32)
    ok(lib.dinox_mae_gather_unfold(P(x), P(ids), P(u), V, H, W, p, Lk, ld, int(bf16), stream()))
    o.fin()
    return u


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("H,W,p", MO.UNFOLD_HWP)
def test_gather_unfold(lib, H, W, p, bf16):
    from dinox import ops
    L, K = (H // p) * (W // p), 3 * p * p
    key = (2, H, W, p, max(L // 4, 1), 8, 1)
    c = case(*key)
    V, Lk = 2, c["dims"][5]
    dt = BF16 if bf16 else F32
    cols = ops.patch_cols(p, dt)
    variants = [(K, None), (K + 16, None), (K, "x"), (K, "u"), (K, "ids_keep")] + ([(50, None)] if p == 4 else []) + ([(cols, None)] if cols != K else [])
    for ld, off in variants:
        want = oracle(("unfold", key, ld), lambda: MO.gather_unfold(c["imgs"], c["ids_keep"], p, ld).astype(np.float32))
        u = run_gather_unfold(lib, c, ld, bf16, off)
        got = npf(u)
        assert np.array_equal(got, bf(want, bf16)), (ld, off)
        assert not got[:, K:].any()                                            # the tail is exactly 0
        if ld == cols and off is None:                                         # rows v L + ids_keep of patch_unfold, bit for bit
            full = ops.patch_unfold(torch.from_numpy(c["imgs"]).to(DEV), p, dt)
            rows = (np.arange(V)[:, None] * L + c["ids_keep"]).reshape(-1)
            assert full.shape == (V * L, cols) and torch.equal(u, full[torch.from_numpy(rows).to(DEV)])


# ------------------------------------------------------------------------------------------ tokens
def run_tokens(lib, c, bf16, off=None, ids_keep=None, ids_restore=None):
    V, H, W, p, L, Lk, D, K = c["dims"]
    dt = BF16 if bf16 else F32
    o = Operands(off)
    patches, cls, pos = o.inp("patches", c["patches"], dt), o.inp("cls", c["cls"]), o.inp("pos", c["pos"])
    ik = o.inp("ids_keep", c["ids_keep"] if ids_keep is None else ids_keep, I32)
    ir = o.inp("ids_restore", c["ids_restore"] if ids_restore is None else ids_restore, I32)
    tok = o.out("tokens", (V, 1 + Lk, D))
    ok(lib.dinox_mae_tokens_fwd(P(patches), P(cls), P(pos), P(ik), P(tok), V, L, Lk, D, int(bf16), stream()))
    gtok = o.inp("dtokens", c["gtok"])
    dp, dcls, dpos = o.out("dpatches", (V, Lk, D), dt), o.out("dcls", (D,)), o.out("dpos", (1 + L, D))
    ok(lib.dinox_mae_tokens_bwd(P(gtok), P(ir), P(dp), P(dcls), P(dpos), V, L, Lk, D, int(bf16), stream()))
    o.fin()
    return npf(tok), npf(dp), npf(dcls), npf(dpos)


def check_tokens(lib, key, bf16, off=None):
    c = case(*key)
    V, H, W, p, L, Lk, D, K = c["dims"]
    tok, dp, dcls, dpos = run_tokens(lib, c, bf16, off)
    want_tok = oracle(("tok", key, bf16), lambda: MO.tokens_fwd(bf(c["patches"], bf16), c["cls"], c["pos"], c["ids_keep"]).astype(np.float32))
    assert np.array_equal(tok, want_tok)                                       # one fp32 add of two fp32 values: float64 then one rounding
    o_dp, o_dcls, o_dpos = oracle(("tokb", key), lambda: MO.tokens_bwd(c["gtok"], c["ids_restore"], Lk))
    assert np.array_equal(dp, bf(o_dp.astype(np.float32), bf16))
    b = oracle(("tokbound", key), lambda: MO.bound_dpos(c["gtok"], c["ids_restore"], Lk))
    within("tokens_bwd.dpos", dpos, o_dpos, b)
    within("tokens_bwd.dcls", dcls, o_dcls, b[0])
    assert np.array_equal(dcls, dpos[0])
    n, _ = MO.tokens_bwd_terms(c["gtok"], c["ids_restore"], Lk)
    assert not dpos[n == 0].any()                                              # positions nobody keeps: exactly 0


def run_unshuffle(lib, c, bf16, off=None, ids_keep=None, ids_restore=None):
    V, H, W, p, L, Lk, D, K = c["dims"]
    dt = BF16 if bf16 else F32
    o = Operands(off)
    e, mt, dpe = o.inp("e", c["e"], dt), o.inp("mask_token", c["mask_token"]), o.inp("dec_pos", c["dec_pos"])
    ik = o.inp("ids_keep", c["ids_keep"] if ids_keep is None else ids_keep, I32)
    ir = o.inp("ids_restore", c["ids_restore"] if ids_restore is None else ids_restore, I32)
    xd = o.out("xd", (V, 1 + L, D))
    ok(lib.dinox_mae_unshuffle_fwd(P(e), P(mt), P(dpe), P(ir), P(xd), V, L, Lk, D, int(bf16), stream()))
    g = o.inp("g", c["gxd"])
    de, dm, ws = o.out("de", (V, 1 + Lk, D), dt), o.out("dmask_token", (D,)), o.out("ws", (V, D))
    ok(lib.dinox_mae_unshuffle_bwd(P(g), P(ik), P(ir), P(de), P(dm), P(ws), V, L, Lk, D, int(bf16), stream()))
    o.fin()
    return npf(xd), npf(de), npf(dm)


def check_unshuffle(lib, key, bf16, off=None):
    c = case(*key)
    V, H, W, p, L, Lk, D, K = c["dims"]
    xd, de, dm = run_unshuffle(lib, c, bf16, off)
    want = oracle(("xd", key, bf16), lambda: MO.unshuffle_fwd(bf(c["e"], bf16), c["mask_token"], c["dec_pos"], c["ids_restore"]).astype(np.float32))
    assert np.array_equal(xd, want)
    o_de, o_dm = oracle(("unb", key), lambda: MO.unshuffle_bwd(c["gxd"], c["ids_keep"], c["ids_restore"]))
    assert np.array_equal(de, bf(o_de.astype(np.float32), bf16))
    within("unshuffle_bwd.dmask_token", dm, o_dm, oracle(("unbound", key), lambda: MO.bound_dmask(c["gxd"], c["ids_restore"], Lk)))


@pytest.mark.parametrize("D", MO.TOKEN_D)
@pytest.mark.parametrize("L,Lk", MO.TOKEN_LLK)
def test_tokens_and_unshuffle(lib, L, Lk, D):
    for V in MO.TOKEN_V:
        for bf16 in (False, True):
            key = (V, 1, L, 1, Lk, D, 2)
            check_tokens(lib, key, bf16)
            check_unshuffle(lib, key, bf16)


@pytest.mark.parametrize("off", ["patches", "cls", "pos", "tokens", "dtokens", "dpatches", "dcls", "dpos", "ids_keep", "ids_restore"])
def test_tokens_with_one_operand_off_alignment(lib, off):
    for bf16 in (False, True):
        check_tokens(lib, (5, 1, 257, 1, 64, 8, 2), bf16, off)


@pytest.mark.parametrize("off", ["e", "mask_token", "dec_pos", "xd", "g", "de", "dmask_token", "ws", "ids_keep", "ids_restore"])
def test_unshuffle_with_one_operand_off_alignment(lib, off):
    for bf16 in (False, True):
        check_unshuffle(lib, (5, 1, 257, 1, 64, 8, 2), bf16, off)


# ------------------------------------------------------------------------------------------ loss
def run_loss(lib, c, lead, pdt, ddt, gscale=1.0, off=None, ids_restore=None, fwd=True):
    """-> (loss, row_loss [V, L] read back from ws, dpred [V, lead + L, K])."""
    V, H, W, p, L, Lk, D, K = c["dims"]
    full = np.concatenate([np.full((V, lead, K), 3.0, np.float32), c["pred"]], axis=1)
    o = Operands(off)
    pred, x = o.inp("pred", full, pdt), o.inp("x", c["imgs"])
    ir = o.inp("ids_restore", c["ids_restore"] if ids_restore is None else ids_restore, I32)
    loss = rows = None
    if fwd:
        loss_t, ws = o.out("loss", (1,)), o.out("ws", (V, L))
        ok(lib.dinox_mae_loss_fwd(P(pred), P(x), P(ir), P(loss_t), P(ws), V, H, W, p, Lk, lead, int(pdt == BF16), stream()))
    dpred = o.out("dpred", (V, lead + L, K), ddt)
    ok(lib.dinox_mae_loss_bwd(P(pred), P(x), P(ir), P(dpred), float(gscale), V, H, W, p, Lk, lead, int(pdt == BF16), int(ddt == BF16), stream()))
    o.fin()
    if fwd:
        loss, rows = float(loss_t.cpu()[0]), npf(ws)
    return loss, rows, dpred


def check_loss(lib, key, lead, bf16, off=None):
    """Forward and fp32 gradient of one case: row_loss, loss and dpred inside their bounds, exact zeros, gscale, two runs, the bf16 gradient."""
    c = case(*key)
    V, H, W, p, L, Lk, D, K = c["dims"]
    pdt = BF16 if bf16 else F32
    vw_f, vw_b = MO.loss_vw(p, off != "pred"), MO.loss_vw(p, off not in ("pred", "dpred"))      # the two launch predicates
    tag_f, tag_b = ("vec" if vw_f == 4 else "scalar"), ("vec" if vw_b == 4 else "scalar")
    pred = bf(c["pred"], bf16)
    o_rows, o_loss, o_d = oracle(("loss", key, bf16), lambda: (MO.loss_rows(pred, c["imgs"], c["ids_restore"], Lk, p),
                                                              MO.loss_fwd(pred, c["imgs"], c["ids_restore"], Lk, p),
                                                              MO.loss_bwd(pred, c["imgs"], c["ids_restore"], Lk, p, 1.0)))
    loss, rows, dpred = run_loss(lib, c, lead, pdt, F32, 1.0, off)
    within(f"loss_fwd.row_loss[{tag_f}]", rows, o_rows, MO.bound_row_loss(o_rows, p, vw_f))
    within(f"loss_fwd.loss[{tag_f}]", loss, o_loss, MO.bound_loss(o_loss, p, vw_f, V * L))
    kept = ~MO.removed_mask(c["ids_restore"], Lk)
    d = npf(dpred)
    assert not rows[kept].any() and not d[:, :lead].any() and not d[:, lead:][kept].any()     # exactly 0 on kept patches and lead rows
    assert (rows[~kept] > 0).all()
    within(f"loss_bwd.dpred[{tag_b}]", d[:, lead:], o_d, MO.bound_dpred(o_d))
    loss2, rows2, dpred2 = run_loss(lib, c, lead, pdt, F32, 1.0, off)
    assert loss2 == loss and np.array_equal(rows, rows2) and torch.equal(dpred, dpred2)       # two runs, the same bits
    _, _, dh = run_loss(lib, c, lead, pdt, F32, 0.5, off, fwd=False)
    within("loss_bwd.dpred[gscale 0.5]", npf(dh)[:, lead:], 0.5 * o_d, MO.bound_dpred(0.5 * o_d))
    _, _, d16 = run_loss(lib, c, lead, pdt, BF16, 1.0, off, fwd=False)
    assert torch.equal(d16, dpred.to(BF16))                                                   # the RNE image of the fp32 result


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("H,W,p", MO.LOSS_HWP)
def test_loss_and_gradient(lib, H, W, p, lead, bf16):
    L = (H // p) * (W // p)
    check_loss(lib, (3, H, W, p, max(L // 4, 1), 8, 3), lead, bf16)


@pytest.mark.parametrize("off", ["pred", "dpred", "x", "ids_restore"])
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_loss_with_one_operand_off_alignment(lib, bf16, off):
    """p = 16 (K = 768): pred one element off takes the scalar kernels, three trips; dpred off the scalar backward alone."""
    check_loss(lib, (3, 32, 48, 16, 1, 8, 3), 1, bf16, off)


def test_loss_mean_over_more_than_1024_rows(lib):
    H, W, p = MO.LOSS_MEAN_HWP
    check_loss(lib, (3, H, W, p, 100, 8, 3), 0, False)


# ------------------------------------------------------------------------------------------ the capped grid's second trip
def test_grid_stride_second_trip(lib):
    """Just over 4096 * 256 work items, not a multiple: every grid-stride loop takes a second, partial trip.  All outputs exact."""
    key = MO.STRIDE_TOKENS
    c = case(*key)
    V, H, W, p, L, Lk, D, K = c["dims"]
    for total in (V * (1 + Lk) * (D // 4), V * Lk * (D // 4), V * (1 + L) * (D // 4)):
        assert MO.GRID_CAP * MO.THREADS < total < 2 * MO.GRID_CAP * MO.THREADS
    check_tokens(lib, key, False)
    check_unshuffle(lib, key, False)
    ukey = MO.STRIDE_UNFOLD
    cu = case(*ukey)
    V, H, W, p, L, Lk, D, K = cu["dims"]
    assert MO.GRID_CAP * MO.THREADS < V * Lk * (K // 4) < 2 * MO.GRID_CAP * MO.THREADS
    u = run_gather_unfold(lib, cu, K, True)
    assert np.array_equal(npf(u), MO.bf16_round(MO.gather_unfold(cu["imgs"], cu["ids_keep"], p, K).astype(np.float32)))


# ------------------------------------------------------------------------------------------ indices out of range
def test_out_of_range_indices_are_clamped_or_removed(lib):
    """ids_restore entries outside [0, Lk) count as removed, ids_keep entries are clamped into [0, L) (include/dinox.h): the results are
    the oracle's under that reading, and no canary around any operand moves (Operands.fin)."""
    key = (3, 28, 42, 14, 2, 8, 7)
    c = case(*key)
    V, H, W, p, L, Lk, D, K = c["dims"]
    ir = c["ids_restore"].copy()
    ir[0, :5] = [-1, Lk, L, 2 ** 31 - 1, -2 ** 31]
    ir[2, L - 1] = -1
    ik = c["ids_keep"].copy()
    ik[0, :2] = [-1, L]
    ik[1, :2] = [2 ** 31 - 1, -2 ** 31]
    ikc = MO.clamp_keep(ik, L)
    for bf16 in (False, True):
        u = run_gather_unfold(lib, c, K, bf16, ids_keep=ik)
        assert np.array_equal(npf(u), bf(MO.gather_unfold(c["imgs"], ikc, p, K).astype(np.float32), bf16))
        tok, dp, dcls, dpos = run_tokens(lib, c, bf16, ids_keep=ik, ids_restore=ir)
        assert np.array_equal(tok, MO.tokens_fwd(bf(c["patches"], bf16), c["cls"], c["pos"], ikc).astype(np.float32))
        o_dp, o_dcls, o_dpos = MO.tokens_bwd(c["gtok"], ir, Lk)
        assert np.array_equal(dp, bf(o_dp.astype(np.float32), bf16))
        within("tokens_bwd.dpos", dpos, o_dpos, MO.bound_dpos(c["gtok"], ir, Lk))
        xd, de, dm = run_unshuffle(lib, c, bf16, ids_keep=ik, ids_restore=ir)
        assert np.array_equal(xd, MO.unshuffle_fwd(bf(c["e"], bf16), c["mask_token"], c["dec_pos"], ir).astype(np.float32))
        o_de, o_dm = MO.unshuffle_bwd(c["gxd"], ikc, ir)
        assert np.array_equal(de, bf(o_de.astype(np.float32), bf16))
        within("unshuffle_bwd.dmask_token", dm, o_dm, MO.bound_dmask(c["gxd"], ir, Lk))
        pred = bf(c["pred"], bf16)
        _, rows, dpred = run_loss(lib, c, 1, BF16 if bf16 else F32, F32, ids_restore=ir)
        o_rows = MO.loss_rows(pred, c["imgs"], ir, Lk, p)
        within("loss_fwd.row_loss[vec]", rows, o_rows, MO.bound_row_loss(o_rows, p, MO.loss_vw(p)))
        # the divisor stays V (L - Lk), whatever the ids say: the oracle's gradient, rescaled from its count of removed patches
        o_d = MO.loss_bwd(pred, c["imgs"], ir, Lk, p) * (MO.removed_mask(ir, Lk).sum() / (V * (L - Lk)))
        within("loss_bwd.dpred[vec]", npf(dpred)[:, 1:], o_d, MO.bound_dpred(o_d))


# ------------------------------------------------------------------------------------------ the Python wrappers
def test_wrappers_equal_the_raw_calls_on_a_rectangular_image(lib):
    from dinox import ops
    key = (3, 28, 42, 14, 1, 8, 3)
    c = case(*key)
    V, H, W, p, L, Lk, D, K = c["dims"]
    t = lambda name, dt=None: torch.from_numpy(c[name]).to(DEV) if dt is None else torch.from_numpy(c[name]).to(DEV).to(dt)
    u = ops.mae_gather_unfold(t("imgs"), t("ids_keep"), p, F32)
    assert torch.equal(u, run_gather_unfold(lib, c, K, False))
    loss, saved = ops.mae_loss_fwd(t("pred"), t("imgs"), t("ids_restore"), Lk, p, 0)
    raw_loss, _, raw_d = run_loss(lib, c, 0, F32, F32)
    assert float(loss) == raw_loss and torch.equal(ops.mae_loss_bwd(saved, 1.0), raw_d)
    e, mt = t("e").requires_grad_(True), t("mask_token").view(1, 1, -1).requires_grad_(True)
    xd = ops.MaeUnshuffleFn.apply(e, mt, t("dec_pos")[None], t("ids_restore"), t("ids_keep"))
    xd.backward(t("gxd"))
    raw_xd, raw_de, raw_dm = run_unshuffle(lib, c, False)
    assert np.array_equal(npf(xd), raw_xd) and np.array_equal(npf(e.grad), raw_de) and np.array_equal(npf(mt.grad).reshape(-1), raw_dm)


def test_zz_report_error_to_bound_ratios():
    for name, r in sorted(RATIOS.items()):
        print(f"max error / bound  {name:34s} {r:.3f}")
    assert RATIOS and max(RATIOS.values()) <= 1.0
