"""csrc/koleo.hip and dinox_normalize_bwd on the device, element by element against oracle/koleo_bounds.py, through the C ABI: every
kernel on the arrays the test hands it (a G it builds, hand-made ties, hand-made idx_all / dist_all), and the chain end to end on the
library's own G.  Every output starts as NaN (integers: a sentinel), every buffer lies between two guard regions that must come back
bit-identical, the padding columns of G hold NaN (in the tie cases 1e30, which would win the search if read), and every case is
launched twice and must repeat bit for bit.

Each check prints ``ratio <kernel> <largest error / bound>`` (visible with ``pytest -s``); the table in DESIGN.md ("KoLeo bounds")
is the per-kernel maximum of those lines."""
import numpy as np
import pytest
import torch

import _small_kernels_oracle as SO
from oracle import koleo_bounds as KB

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 256                                                              # elements on both sides of every buffer
CANARY = 0x7A5C3CA5                                                      # a bit pattern no test value has (fp32 2.9e35)
SENTINEL = -777
F32 = np.float32


@pytest.fixture(scope="module")
def L():
    import dinox._lib as lib
    assert lib.lib.dinox_device_ok() == 1, lib.last_error()
    return lib


class Buf:
    """values (an input) or a shape (an output, filled with NaN / the sentinel) between two guard regions; shift: elements by which
    the payload starts off a 16-byte boundary."""

    def __init__(self, values=None, shape=None, dtype=torch.float32, shift=0):
        if values is not None:
            values = torch.as_tensor(np.ascontiguousarray(values))
            shape, dtype = tuple(values.shape), values.dtype
        n = int(np.prod(shape))
        self.raw = torch.full((n + 2 * GUARD + shift,), CANARY, dtype=torch.int32, device=DEV)
        self.lo, self.hi = GUARD + shift, GUARD + shift + n
        self.t = self.raw[self.lo:self.hi].view(dtype).view(shape)
        if values is not None:
            self.t.copy_(values)
        elif dtype == torch.int32:
            self.t.fill_(SENTINEL)
        else:
            self.t.fill_(float("nan"))
        self.is_input = values is not None
        self.before = self.raw.clone()
        assert (self.t.data_ptr() % 16 != 0) == (shift % 4 != 0)

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


def stream():
    return torch.cuda.current_stream().cuda_stream


def twice(launch, ins, make_outs):
    """Launch into two fresh sets of outputs: both must be bit-identical, every guard intact, no NaN or sentinel left."""
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
        assert not (a.t == SENTINEL).any() if a.t.dtype == torch.int32 else bool(torch.isfinite(a.t).all()), "an output element was not written"
    return [o.np() for o in runs[0]]


def within(name, got, ref, bound):
    c = KB.check(got, ref, bound)
    print(f"ratio {name} {c['ratio']:.4f}")
    assert c["nan"] == 0 and c["ratio"] <= 1.0, (name, c)
    return c["ratio"]


# ------------------------------------------------------------------------------------------ each kernel on handed arrays
def run_normalize(L, x):
    V, D = x.shape
    xin = Buf(x)
    xh, norm, sq = twice(lambda a, b, c: L.check(L.lib.dinox_koleo_normalize(xin.p, a.p, b.p, c.p, V, D, 1e-12, stream()), "koleo_normalize"),
                         [xin], lambda: (Buf(shape=(V, D)), Buf(shape=(V,)), Buf(shape=(V,))))
    return xh, norm, sq


@pytest.mark.parametrize("D", KB.WIDTHS + (KB.WIDE,))
def test_normalize(L, D):
    """One, two and more trips of the 256-thread stride and their ragged ends; the clamp and the all-zero row have their own statements."""
    for family in KB.FAMILIES:
        x = KB.make_rows(family, 6, D)
        xh, norm, sq = run_normalize(L, x)
        r = KB.normalize_ref(x)
        for k, v in (("xh", xh), ("norm", norm), ("sq", sq)):
            within(f"normalize.{k} {family} D={D}", v, r[k], r[k + "_bound"])
        if family.startswith("zero"):
            assert (xh[2] == 0).all() and sq[2] == 0 and norm[2] == 0
        if family == "tiny":
            assert r["clamped"].tolist() == [False, True] + [False] * 4 and 0.009 < sq[1] < 0.011


def run_nn(L, G, sq, xh, row0, pad=5, fill=np.nan):
    V_l, V_g = G.shape
    D = xh.shape[1]
    Gp = np.full((V_l, V_g + pad), fill, dtype=F32)
    Gp[:, :V_g] = G
    ins = [Buf(Gp), Buf(sq), Buf(xh)]
    return twice(lambda i, d: L.check(L.lib.dinox_koleo_nn(ins[0].p, V_g + pad, ins[1].p, ins[2].p, row0, V_l, V_g, D, i.p, d.p, stream()), "koleo_nn"),
                 ins, lambda: (Buf(shape=(V_l,), dtype=torch.int32), Buf(shape=(V_l,))))


@pytest.mark.parametrize("V_l,V_g,row0", [(v, v, 0) for v in KB.NN_SIZES] + list(KB.RECT))
def test_nn(L, V_l, V_g, row0):
    """G is the float64 product rounded once: idx exactly the float32 rule, dist relative, the pick within the selection contract."""
    xh = KB.unit_rows(V_g, 16)
    G, sq = KB.gram32(xh[row0:row0 + V_l], xh), KB.sq32(xh)
    idx, dist = run_nn(L, G, sq, xh, row0)
    want = KB.nn_index(G, sq, row0)
    assert (idx == want).all(), np.nonzero(idx != want)[0][:8]
    ref, bound = KB.nn_dist_ref(xh, want, row0)
    within(f"nn.dist {V_l}x{V_g} row0={row0}", dist, ref, bound)
    if V_g == 1:
        assert idx[0] == -1 and dist[0] == KB.NO_NEIGHBOUR
    else:
        sqf = sq.astype(np.float64)
        c = KB.selection_contract(idx, G, sq, xh, row0, KB.U32 * sqf, KB.U32 * np.abs(G.astype(np.float64)))
        within(f"nn.contract {V_l}x{V_g} row0={row0}", c["ratio"], 0.0, 1.0)


@pytest.mark.parametrize("D", [3, 257])
def test_nn_close_rows(L, D):
    """Rows at 1e3 x a common vector and planted pairs down to d = 1e-4: the distance keeps its digits, the pick keeps the contract."""
    for family in ("offset", "pairs", "cluster", "dup"):
        xh = run_normalize(L, KB.make_rows(family, 300, D))[0]
        G, sq = KB.gram32(xh, xh), KB.sq32(xh)
        idx, dist = run_nn(L, G, sq, xh, 0)
        want = KB.nn_index(G, sq, 0)
        assert (idx == want).all()
        ref, bound = KB.nn_dist_ref(xh, want, 0)
        within(f"nn.dist {family} D={D}", dist, ref, bound)
        c = KB.selection_contract(idx, G, sq, xh, 0, KB.U32 * sq.astype(np.float64), KB.U32 * np.abs(G.astype(np.float64)))
        within(f"nn.contract {family} D={D}", c["ratio"], 0.0, 1.0)


@pytest.mark.parametrize("mode", KB.TIE_MODES)
def test_nn_exact_ties(L, mode):
    """The lowest index of an exact tie, across waves, across a thread's two visits, at the last column and around the diagonal,
    which holds the smallest value of all and is excluded."""
    for V_l, V_g, row0 in [(100, 700, 300), (100, 700, 0), (700, 700, 0)]:
        G, sq, want = KB.tie_case(mode, V_l, V_g, row0)
        xh = KB.unit_rows(V_g, 16)
        idx, dist = run_nn(L, G, sq, xh, row0, fill=1e30)                # padding that would win the search if it were read
        assert (idx == want).all(), (mode, V_l, row0, np.nonzero(idx != want)[0][:8])
        ref, bound = KB.nn_dist_ref(xh, want, row0)
        within(f"nn.dist ties/{mode} {V_l}x{V_g} row0={row0}", dist, ref, bound)


@pytest.mark.parametrize("V", KB.LOSS_SIZES)
def test_loss(L, V):
    d = np.abs(np.random.default_rng(V).standard_normal(V)).astype(F32)
    d[0] = 0.0
    d[V // 2] = 0.0 if V == 1 else 1e9
    din = Buf(d)
    (out,) = twice(lambda o: L.check(L.lib.dinox_koleo_loss(din.p, V, 1e-8, o.p, stream()), "koleo_loss"), [din], lambda: (Buf(shape=(1,)),))
    ref, bound = KB.loss_ref(d, log_rtol=SO.CE_LOSS_RTOL)
    within(f"loss V={V}", out[0], ref, bound)


def run_bwd(L, c):
    ins = [Buf(c["xh_all"]), Buf(c["idx_all"]), Buf(c["dist_all"]), Buf(c["norm_loc"])]
    (dx,) = twice(lambda o: L.check(L.lib.dinox_koleo_bwd(ins[0].p, ins[1].p, ins[2].p, ins[3].p, c["row0"], c["V_l"], c["V_g"], c["D"],
                                                            c["gscale"], 1e-8, 1e-12, o.p, stream()), "koleo_bwd"),
                  ins, lambda: (Buf(shape=(c["V_l"], c["D"])),))
    ref = KB.bwd_ref(c["xh_all"], c["idx_all"], c["dist_all"], c["norm_loc"], c["row0"], c["gscale"])
    return dx, ref


@pytest.mark.parametrize("name", KB.BWD_CASES)
def test_bwd(L, name):
    c = KB.bwd_case(name)
    dx, ref = run_bwd(L, c)
    within(f"bwd {name} n_in<={int(ref['n_in'].max())}", dx, ref["dx"], ref["dx_bound"])


def test_bwd_neighbour_list_limit(L):
    """15359 rows fill the 60 KiB list and are served; 15360 are refused and dx is left as it was."""
    V_g, D, V_l = KB.MAX_LIST_ROWS, 4, 2
    xh = KB.unit_rows(V_g, D)
    idx = np.zeros(V_g, dtype=np.int32)                                  # row 0 is chosen by every other row: the list is full
    idx[0] = 1
    x64 = xh.astype(np.float64)
    dist = np.sqrt(((x64 - x64[idx]) ** 2).sum(1)).astype(F32)
    c = {"xh_all": xh, "idx_all": idx, "dist_all": dist, "norm_loc": np.array([2.0, 0.5], dtype=F32), "row0": 0, "V_l": V_l, "V_g": V_g,
         "D": D, "gscale": float(F32(0.37))}
    dx, ref = run_bwd(L, c)
    assert ref["n_in"][0] == V_g - 1
    within(f"bwd limit V_g={V_g}", dx, ref["dx"], ref["dx_bound"])
    big = [Buf(KB.unit_rows(V_g + 1, D)), Buf(np.zeros(V_g + 1, dtype=np.int32)), Buf(np.ones(V_g + 1, dtype=F32)), Buf(c["norm_loc"])]
    out = Buf(shape=(V_l, D))
    rc = L.lib.dinox_koleo_bwd(big[0].p, big[1].p, big[2].p, big[3].p, 0, V_l, V_g + 1, D, 1.0, 1e-8, 1e-12, out.p, stream())
    torch.cuda.synchronize()
    assert rc == L.EUNSUPPORTED == -2 and "neighbour list" in L.last_error()
    assert torch.equal(out.raw, out.before)


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "off1"])
@pytest.mark.parametrize("D", KB.NBWD_WIDTHS)
def test_normalize_bwd(L, D, shift):
    """float4 kernel (D % 4 == 0, aligned) and scalar kernel (any other D, or pointers one float off alignment)."""
    dxh, xh, norm = KB.nbwd_case(D)
    V = len(norm)
    ins = [Buf(dxh, shift=shift), Buf(xh, shift=shift), Buf(norm)]
    (dx,) = twice(lambda o: L.check(L.lib.dinox_normalize_bwd(ins[0].p, ins[1].p, ins[2].p, o.p, V, D, 1e-12, stream()), "normalize_bwd"),
                  ins, lambda: (Buf(shape=(V, D), shift=shift),))
    vec = D % 4 == 0 and shift == 0
    ref, bound = KB.normalize_bwd_ref(dxh, xh, norm, vec=vec)
    within(f"normalize_bwd.{'vec' if vec else 'scalar'} D={D} shift={shift}", dx, ref, bound)


# ------------------------------------------------------------------------------------------ end to end on the library's G
def e2e_run(ops, x, gscale):
    state = ops.koleo_begin(x)
    xh, xh_all, sq_all, norm = state[:4]
    G = ops.gemm_nt_f32_splitk(xh, xh_all)
    loss, saved = ops.koleo_end(state)
    dx = ops.koleo_bwd(saved, gscale)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (xh, norm, sq_all, G, saved[1], saved[2], loss, dx)]


@pytest.mark.parametrize("V,D", KB.E2E)
@pytest.mark.parametrize("family", KB.E2E_FAMILIES)
def test_end_to_end(L, family, V, D):
    """ops.koleo_fwd / koleo_bwd (its two halves, so that the library's own G can be read): every stage given the stage before.  The
    gradients of the duplicates (d = 0) and of the all-zero row are compared element by element like every other row."""
    from dinox import ops
    x = KB.make_rows(family, V, D, seed=KB.e2e_seed(family, V, D))
    xd = torch.from_numpy(x).to(DEV)
    gscale = 0.1
    a, b = e2e_run(ops, xd, gscale), e2e_run(ops, xd, gscale)
    assert all(p.tobytes() == q.tobytes() for p, q in zip(a, b)), "a second run differs"
    xh, norm, sq, G, idx, dist, loss, dx = a
    tag = f"{family} {V}x{D}"
    r = KB.normalize_ref(x)
    for k, v in (("xh", xh), ("norm", norm), ("sq", sq)):
        within(f"e2e.normalize.{k} {tag}", v, r[k], r[k + "_bound"])
    want = KB.nn_index(G, sq, 0)
    assert (idx == want).all(), np.nonzero(idx != want)[0][:8]
    ref, bound = KB.nn_dist_ref(xh, want, 0)
    within(f"e2e.nn.dist {tag}", dist, ref, bound)
    e_sq, e_g = KB.handed_errors(xh, xh, D + max(1, D // 256))
    c = KB.selection_contract(idx, G, sq, xh, 0, e_sq, e_g)
    within(f"e2e.nn.contract {tag}", c["ratio"], 0.0, 1.0)
    differ = (c["d2"][np.arange(V), idx] > c["d2"][np.arange(V), c["near"]]) & (xh != 0).any(1)
    print(f"share {tag} {differ.mean():.4f} excess {c['excess']:.3e} "
          f"loss-term {np.abs(np.log(np.sqrt(c['d2'][np.arange(V), idx]) + 1e-8) - np.log(np.sqrt(c['d2'].min(1)) + 1e-8)).max():.3e}")
    if family not in KB.SHARE_EXEMPT:                                    # cluster, and offset at 1e3: the contract alone judges the pick
        assert not differ.any(), np.nonzero(differ)[0][:8]
    lref, lbound = KB.loss_ref(dist, log_rtol=SO.CE_LOSS_RTOL)
    within(f"e2e.loss {tag}", loss[0], lref, lbound)
    bref = KB.bwd_ref(xh, idx, dist, norm, 0, gscale / V)
    within(f"e2e.bwd {tag} n_in<={int(bref['n_in'].max())}", dx, bref["dx"], bref["dx_bound"])
    if family == "dup":
        assert dist[0] == 0 and dist[1] == 0 and dist[2] == 0 and np.isfinite(dx[:3]).all()
