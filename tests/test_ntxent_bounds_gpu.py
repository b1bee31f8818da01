"""csrc/ntxent.hip on the device, element by element against oracle/ntxent_bounds.py, through the C ABI: dinox_ntxent_rows,
dinox_ntxent_coeff and their rectangular forms on an S the test builds (asymmetric, duplicated, collapsed, one-hot, antipodal, with
zero rows; tau down to 0.01), the shard identity on one device, and ops.ntxent_fwd / ntxent_bwd end to end.  Every excluded entry of S
holds NaN (once per shape 1e30, which would win the maximum if read) and so does every padding column; every output starts as NaN,
every buffer lies between two guard regions that must come back bit-identical, the padding columns of W are canaries, and every case
is launched twice into fresh outputs and must repeat bit for bit.

Each check prints ``NTXENT-BOUNDS <kernel> <family> <shape> tau=...: ratio=...`` (visible with ``pytest -s``); the table in
DESIGN.md ("NT-Xent bounds") is the per-kernel maximum that test_zz_report_error_to_bound_ratios prints."""
import math

import numpy as np
import pytest
import torch

import _small_kernels_oracle as SO
from oracle import ntxent_bounds as NB

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 256                                                              # elements on both sides of every buffer
CANARY = 0x7A5C3CA5                                                      # NB.CANARY as a word
F32, F64 = np.float32, np.float64
WORST = {}
COMPARED = {}


@pytest.fixture(scope="module")
def L():
    import dinox._lib as lib
    assert lib.lib.dinox_device_ok() == 1, lib.last_error()
    assert NB.EXP_LOG_RTOL == SO.CE_LOSS_RTOL
    return lib


class Buf:
    """values (an input) or a shape (an output, filled with NaN; live: the columns of a W that may be written, the padding columns
    beyond them keep the guard word and must survive) between two guard regions."""

    def __init__(self, values=None, shape=None, live=None):
        if values is not None:
            values = torch.as_tensor(np.ascontiguousarray(values, dtype=F32))
            shape = tuple(values.shape)
        n = int(np.prod(shape))
        self.raw = torch.full((n + 2 * GUARD,), CANARY, dtype=torch.int32, device=DEV)
        self.lo, self.hi = GUARD, GUARD + n
        self.t = self.raw[self.lo:self.hi].view(torch.float32).view(shape)
        if values is not None:
            self.t.copy_(values)
        else:
            self.t[..., :live].fill_(float("nan"))
        self.is_input = values is not None
        self.before = self.raw.clone()

    @property
    def p(self):
        return self.t.data_ptr()

    def np(self):
        return self.t.cpu().numpy()

    def intact(self):
        """The guards (and, for an input, the payload) are bit-identical to what they were."""
        if self.is_input:
            return torch.equal(self.raw, self.before)
        return torch.equal(self.raw[:self.lo], self.before[:self.lo]) and torch.equal(self.raw[self.hi:], self.before[self.hi:])

    def untouched(self):
        return torch.equal(self.raw, self.before)


def stream():
    return torch.cuda.current_stream().cuda_stream


def twice(launch, ins, make_outs):
    """Launch into two fresh sets of outputs: both must be bit-identical and every guard and input intact."""
    runs = []
    for _ in range(2):
        outs = make_outs()
        launch(*outs)
        torch.cuda.synchronize()
        for b in list(ins) + list(outs):
            assert b.intact(), "a guard region or an input changed"
        runs.append(outs)
    for a, b in zip(*runs):
        assert torch.equal(a.t.view(torch.int32), b.t.view(torch.int32)), "a second launch differs"
    return [o.np() for o in runs[0]]


def hold(kernel, tag, ratio, compared, expected):
    print(f"NTXENT-BOUNDS {kernel} {tag}: ratio={ratio:.4f}")
    assert compared == expected, (kernel, tag, compared, expected)
    assert ratio <= 1.0, (kernel, tag, ratio)                            # (a non-finite element, or a changed canary, is inf)
    WORST[kernel] = max(WORST.get(kernel, 0.0), ratio)
    COMPARED[kernel] = COMPARED.get(kernel, 0) + compared


def run_rows(L, S, lds, Ml, Mg, row0, it, square):
    sin = Buf(S)
    if square:
        call = lambda a, b, c: L.check(L.lib.dinox_ntxent_rows(sin.p, lds, Ml, it, a.p, b.p, c.p, stream()), "ntxent_rows")
    else:
        call = lambda a, b, c: L.check(L.lib.dinox_ntxent_rows_rect(sin.p, lds, Ml, Mg, row0, Ml // 2, it, a.p, b.p, c.p, stream()), "ntxent_rows_rect")
    return twice(call, [sin], lambda: (Buf(shape=(Ml,)), Buf(shape=(Ml,)), Buf(shape=(1,))))


def hold_rows(kernel, tag, got, S, it, Mg, row0, divisor, ref):
    lse, row_loss, out = got
    r = NB.judge_rows(lse, row_loss, out[0], S, it, Mg, row0, divisor, ref)
    for k in ("lse", "row_loss"):
        hold(f"{kernel}.{k}", tag, r[k], got[("lse", "row_loss").index(k)].size, len(ref["lse"]))
    hold(f"{kernel}.loss", tag, max(r["loss"], r["loss_e2e"]), out.size, 1)


def run_coeff(L, S, lds, lse, M, it, gscale, ldw):
    ins = [Buf(S), Buf(lse)]
    (W,) = twice(lambda w: L.check(L.lib.dinox_ntxent_coeff(ins[0].p, lds, ins[1].p, M, it, gscale, w.p, ldw, stream()), "ntxent_coeff"),
                 ins, lambda: (Buf(shape=(M, ldw), live=M),))
    return W


def run_coeff_rect(L, S, lds, lse_local, lse_all, Ml, Mg, row0, it, gscale, ldw):
    ins = [Buf(S), Buf(lse_local), Buf(lse_all)]
    (W,) = twice(lambda w: L.check(L.lib.dinox_ntxent_coeff_rect(ins[0].p, lds, ins[1].p, ins[2].p, Ml, Mg, row0, Ml // 2, it, gscale, w.p, ldw,
                                                                  stream()), "ntxent_coeff_rect"),
                 ins, lambda: (Buf(shape=(Ml, ldw), live=Mg),))
    return W


def hold_w(kernel, tag, W, rows, cols, ldw, ref, gscale):
    body = W.reshape(rows, ldw)[:, :cols]
    diag = ref["W_bound"] == 0.0
    assert (body[diag] == 0.0).all() and not np.signbit(body[diag]).any(), "an excluded entry of W is not +0.0f"
    hold(kernel, tag, NB.judge_w(W.reshape(-1), rows, cols, ldw, ref, gscale), body.size, rows * cols)


# ------------------------------------------------------------------------------------------ the square kernels
@pytest.mark.parametrize("v", NB.VARIANTS)
@pytest.mark.parametrize("tau", NB.TAUS)
@pytest.mark.parametrize("M", NB.SQUARE_M)
def test_rows_and_coeff(L, M, tau, v):
    """dinox_ntxent_rows with lds = M and M + 5; dinox_ntxent_coeff on the lse that launch produced, with ldw = M and M + 3 at
    gscale 1 and 0.25.  258: the second 256-stride holds two columns and the diagonals of the rows from 256 on; 1026: the second pass
    of the sum kernel; 34 and 66: a ragged 2-wide tile in both directions and its mirror."""
    it = NB.f32(1.0 / tau)
    family, fill = NB.variant(v)
    Sg = NB.make_S(family, M)
    rref = cref = lse0 = None
    for pad in (0, NB.LDS_PAD):
        lds = M + pad
        S = NB.poison(Sg, 0, lds, fill)
        rref = NB.rows_ref(S, it, M) if rref is None else rref
        got = run_rows(L, S, lds, M, M, 0, it, True)
        hold_rows("rows", f"{v} M={M} lds={lds} tau={tau}", got, S, it, M, 0, M, rref)
        assert lse0 is None or got[0].tobytes() == lse0.tobytes(), "lse depends on lds"
        lse0 = got[0]
        cref = NB.coeff_ref(S, lse0, it, 1.0, M) if cref is None else cref
        for gscale, wpad in zip(NB.GSCALES, (0, NB.LDW_PAD) if pad else (NB.LDW_PAD, 0)):
            W = run_coeff(L, S, lds, lse0, M, it, gscale, M + wpad)
            hold_w("coeff", f"{v} M={M} lds={lds} ldw={M + wpad} g={gscale} tau={tau}", W, M, M, M + wpad, cref, gscale)


# ------------------------------------------------------------------------------------------ the rectangular kernels
@pytest.mark.parametrize("tau", NB.TAUS)
@pytest.mark.parametrize("Ml,world", NB.RECT)
def test_rows_rect_and_coeff_rect(L, Ml, world, tau):
    """Every row0 of every (Ml, world); distinct lse_local (what the launch before produced) and lse_all (the float64 lse of every
    rank, moved by 0.25 sin j).  (66, 4): Mg = 264 crosses the 256-stride; (2, 3): one pair per rank.  world = 1: lse is the square
    kernel's, bit for bit."""
    it = NB.f32(1.0 / tau)
    Mg = Ml * world
    for n, v in enumerate(NB.VARIANTS):
        family, fill = NB.variant(v)
        Sg = NB.make_S(family, Ml, world)
        lse_all = NB.lse_all_for(Sg, Ml, it)
        for r, row0 in enumerate(range(0, Mg, Ml)):
            pad, wpad = ((0, NB.LDW_PAD), (NB.LDS_PAD, 0))[(n + r) % 2]
            lds, ldw = Mg + pad, Mg + wpad
            gscale = NB.GSCALES[(n + r) % 2]
            S = NB.poison(Sg[row0:row0 + Ml], row0, lds, fill)
            tag = f"{v} {Ml}x{Mg} row0={row0} lds={lds} ldw={ldw} g={gscale} tau={tau}"
            rref = NB.rows_ref(S, it, Mg, row0)
            got = run_rows(L, S, lds, Ml, Mg, row0, it, False)
            hold_rows("rows_rect", tag, got, S, it, Mg, row0, 1.0, rref)
            if world == 1:
                sq = run_rows(L, S, lds, Ml, Ml, 0, it, True)
                assert sq[0].tobytes() == got[0].tobytes() and sq[1].tobytes() == got[1].tobytes(), "world = 1 is not the square kernel"
            W = run_coeff_rect(L, S, lds, got[0], lse_all, Ml, Mg, row0, it, gscale, ldw)
            hold_w("coeff_rect", tag, W, Ml, Mg, ldw, NB.coeff_rect_ref(S, got[0], lse_all, row0, it), gscale)


# ------------------------------------------------------------------------------------------ shards against the global batch
@pytest.mark.parametrize("Ml,world", NB.SHARD)
def test_shards_add_up_to_the_global_batch(L, Ml, world):
    """A global batch [z1 of all ranks; z2 of all ranks] cut into rank blocks on one device.  S is the float64 product moved by one ulp
    at random, so S_ij != S_ji: the rectangular W / world is held to the global W's bound plus |S_ij - S_ji| inv_tau P_ji and the
    response of both exponentials to the two launches' own lse (twice the lse bound each)."""
    tau = 0.1
    it = NB.f32(1.0 / tau)
    Mg = Ml * world
    g = NB.shard_maps(Ml, world)                                         # gathered index r Ml + i -> global row
    flat = g.reshape(-1)
    for family in ("randn", "duplicates", "onehot"):
        z = np.empty((Mg, 32))
        z[flat] = NB.make_z(family, Ml, world)                           # the same rows, in the global order
        rng = np.random.default_rng([53, Ml, world])
        Sglob = (z @ z.T).astype(F32)
        Sglob = np.nextafter(Sglob, np.where(rng.random((Mg, Mg)) < 0.5, F32(-2), F32(2))).astype(F32)
        Sp = NB.poison(Sglob)
        gref = NB.rows_ref(Sp, it)
        glse, grow, gloss = run_rows(L, Sp, Mg, Mg, Mg, 0, it, True)
        cref = NB.coeff_ref(Sp, glse, it, 1.0, Mg)
        lses, parts, Ss = [], [], []
        for r in range(world):
            S = NB.poison(Sglob[g[r]][:, flat], r * Ml)
            lse, row_loss, part = run_rows(L, S, Mg, Ml, Mg, r * Ml, it, False)
            c = NB.check(lse, gref["lse"][g[r]], gref["lse_bound"][g[r]])
            hold("shard.lse", f"{family} {Ml}x{Mg} rank={r}", c["ratio"] if c["nan"] == 0 else math.inf, lse.size, Ml)
            lses.append(lse)
            parts.append(part[0])
            Ss.append(S)
        total = F32(0)
        for p in parts:                                                  # rank order, as ops.ntxent_fwd adds the gathered sums
            total = F32(total + p)
        loss = F32(total / F32(Mg))
        bound = gref["row_loss_bound"].sum() / Mg + (Ml + world + 1 + 2) * NB.U * np.abs(gref["row_loss"]).sum() / Mg + NB.TINY
        hold("shard.loss", f"{family} {Ml}x{Mg}", abs(float(loss) - gref["row_loss"].sum() / Mg) / bound, 1, 1)
        lse_all = np.concatenate(lses)
        x = Sglob.astype(F64) * it
        for r in range(world):
            W = run_coeff_rect(L, Ss[r], Mg, lses[r], lse_all, Ml, Mg, r * Ml, it, 1.0, Mg).reshape(Ml, Mg)
            rows = g[r]
            dl = 2.0 * gref["lse_bound"]
            asym = np.abs(x - x.T)[rows][:, flat]
            extra = it / Mg * (cref["P1"][rows][:, flat] * np.expm1(dl[rows])[:, None]
                               + cref["P2"][rows][:, flat] * np.expm1(dl[flat][None, :] + asym))
            want, wb = cref["W"][rows][:, flat], cref["W_bound"][rows][:, flat]
            c = NB.check(W.astype(F64) / world, want, np.where(wb > 0.0, wb + extra + NB.U * np.abs(want), 0.0))
            hold("shard.W", f"{family} {Ml}x{Mg} rank={r}", c["ratio"] if c["nan"] == 0 else math.inf, W.size, Ml * Mg)


# ------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("D", NB.E2E_D)
@pytest.mark.parametrize("M", NB.E2E_M)
def test_end_to_end(L, M, D):
    """ops.ntxent_fwd / ntxent_bwd and their force_rect twin: loss and every element of dz against _ntxent_oracle.ntxent, within the
    bound carried through normalize, both products, the row pass, W and the backward of the normalisation.  The gradients of the
    duplicated rows and of the two all-zero rows (dz = dzh / eps there) are compared like every other."""
    from dinox import ops
    for family in NB.E2E_FAMILIES:
        z = NB.make_z(family, M, 1, D).astype(F32)
        zd = torch.from_numpy(z).to(DEV)
        for tau in NB.E2E_TAUS:
            for rect in (False, True):
                runs = []
                for _ in range(2):
                    loss, saved = ops.ntxent_fwd(zd.clone(), tau, force_rect=rect)
                    dz = ops.ntxent_bwd(saved, 1.0)
                    torch.cuda.synchronize()
                    runs.append((loss.cpu().numpy(), dz.cpu().numpy()))
                assert all(a.tobytes() == b.tobytes() for a, b in zip(*runs)), "a second run differs"
                ref = NB.e2e_ref(z, NB.f32(1.0 / tau), rect)
                tag = f"{family} {M}x{D} tau={tau}"
                kind = "e2e_rect" if rect else "e2e"
                c = NB.check(runs[0][0], [ref["loss"]], [ref["loss_bound"]])
                hold(f"{kind}.loss", tag, c["ratio"] if c["nan"] == 0 else math.inf, runs[0][0].size, 1)
                c = NB.check(runs[0][1], ref["dz"], ref["dz_bound"])
                hold(f"{kind}.dz", tag, c["ratio"] if c["nan"] == 0 else math.inf, runs[0][1].size, M * D)


# ------------------------------------------------------------------------------------------ refusals
def test_refusals_write_nothing(L):
    M, it = 6, 10.0
    S = Buf(np.zeros((8, 16), dtype=F32))
    lse, lse_all = Buf(np.zeros(8, dtype=F32)), Buf(np.zeros(16, dtype=F32))
    o = [Buf(shape=(8,)), Buf(shape=(8,)), Buf(shape=(1,)), Buf(shape=(8, 16))]
    a, b, c, W = (x.p for x in o)
    lib, st = L.lib, stream()
    calls = {
        "rows odd M": lambda: lib.dinox_ntxent_rows(S.p, 8, 5, it, a, b, c, st),
        "rows lds < M": lambda: lib.dinox_ntxent_rows(S.p, M - 1, M, it, a, b, c, st),
        "rows inv_tau = 0": lambda: lib.dinox_ntxent_rows(S.p, M, M, 0.0, a, b, c, st),
        "rows inv_tau < 0": lambda: lib.dinox_ntxent_rows(S.p, M, M, -it, a, b, c, st),
        "coeff odd M": lambda: lib.dinox_ntxent_coeff(S.p, 8, lse.p, 5, it, 1.0, W, 8, st),
        "coeff lds < M": lambda: lib.dinox_ntxent_coeff(S.p, M - 1, lse.p, M, it, 1.0, W, M, st),
        "coeff ldw < M": lambda: lib.dinox_ntxent_coeff(S.p, M, lse.p, M, it, 1.0, W, M - 1, st),
        "coeff inv_tau = 0": lambda: lib.dinox_ntxent_coeff(S.p, M, lse.p, M, 0.0, 1.0, W, M, st),
        "coeff W == S": lambda: lib.dinox_ntxent_coeff(W, M, lse.p, M, it, 1.0, W, M, st),
        "rows_rect odd Ml": lambda: lib.dinox_ntxent_rows_rect(S.p, 16, 3, 6, 0, 1, it, a, b, c, st),
        "rows_rect lds < Mg": lambda: lib.dinox_ntxent_rows_rect(S.p, 11, M, 12, 0, 3, it, a, b, c, st),
        "rows_rect row0 not a block start": lambda: lib.dinox_ntxent_rows_rect(S.p, 12, M, 12, 3, 3, it, a, b, c, st),
        "rows_rect row0 past the end": lambda: lib.dinox_ntxent_rows_rect(S.p, 12, M, 12, 12, 3, it, a, b, c, st),
        "rows_rect Mg % Ml": lambda: lib.dinox_ntxent_rows_rect(S.p, 16, M, 14, 0, 3, it, a, b, c, st),
        "rows_rect Bl": lambda: lib.dinox_ntxent_rows_rect(S.p, 12, M, 12, 0, 2, it, a, b, c, st),
        "rows_rect inv_tau = 0": lambda: lib.dinox_ntxent_rows_rect(S.p, 12, M, 12, 0, 3, 0.0, a, b, c, st),
        "coeff_rect ldw < Mg": lambda: lib.dinox_ntxent_coeff_rect(S.p, 12, lse.p, lse_all.p, M, 12, 0, 3, it, 1.0, W, 11, st),
        "coeff_rect lds < Mg": lambda: lib.dinox_ntxent_coeff_rect(S.p, 11, lse.p, lse_all.p, M, 12, 0, 3, it, 1.0, W, 12, st),
        "coeff_rect row0 not a block start": lambda: lib.dinox_ntxent_coeff_rect(S.p, 12, lse.p, lse_all.p, M, 12, 4, 3, it, 1.0, W, 12, st),
        "coeff_rect Mg % Ml": lambda: lib.dinox_ntxent_coeff_rect(S.p, 16, lse.p, lse_all.p, M, 14, 0, 3, it, 1.0, W, 14, st),
        "coeff_rect inv_tau < 0": lambda: lib.dinox_ntxent_coeff_rect(S.p, 12, lse.p, lse_all.p, M, 12, 0, 3, -it, 1.0, W, 12, st),
    }
    for name, call in calls.items():
        rc = call()
        torch.cuda.synchronize()
        assert rc == -1 and L.last_error(), name
        assert all(x.untouched() for x in o + [S, lse, lse_all]), name


def test_zz_report_error_to_bound_ratios():
    for k in sorted(WORST):
        print(f"NTXENT-BOUNDS max {k}: ratio={WORST[k]:.4f} over {COMPARED[k]} elements")
