"""GPU tests of the compiled paths of the dense-segmentation kernels that the feature modules leave out: the register widths 16 and 32
and the exact fills C = 4, 8, 16, 32 of every kernel of csrc/segloss.hip, csrc/segcalib.hip, csrc/segrefine.hip and csrc/segblend.hip;
the byte label load and the byte prediction store at the factors where the 32-bit ones are the default (u = 8, 24, 32), and those at cells
12 / 8 / 4, 36 / 24 / 12 and 48 / 32 / 16 wide; the factors 1, 2, 8, 24, 32 through the loss backward and the boundary term; all fifteen
(CP, r) of the refinement's iteration kernel; the ``C == CP`` branch of the blend kernel at every width.

The cases are tests/_seg_paths_cases.py's (tests/test_seg_paths_cpu.py shows that they reach every path and builds their inputs and
oracle objects, once).  Nothing here has a bound or a tolerance of its own: every output is held to the float64 oracle of its kernel --
tests/_segloss_oracle.py, _bdloss_oracle.py, _segcalib_oracle.py, _segrefine_oracle.py, _segblend_oracle.py -- by the conventions of that
kernel's own module: every element compared, no NaN, integers equal, the arg-max where the float64 margin decides, exact zeros under
"all ignored".  Beside that, for every case: a second call gives the same bits; w_bd = 0 gives the bits of the entry points without the
term; T = 0 of the refinement gives seg_predict's map and counts and seg_calib's confidence.

One line per case and kernel: ``SEG-PATHS <kernel> <path> <shape>: ratio=<largest error / bound>``."""
import numpy as np
import pytest
import torch

import _seg_paths_cases as P
import _segblend_oracle as BLO
import _segcalib_oracle as CO
import _segloss_oracle as SO
import test_seg_paths_cpu as L
from test_segloss_gpu import on_device
from test_segrefine_cpu import make_guide

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CANARY = 0xA5
RATIOS: dict = {}


def ratio_of(name, got, ref, bound, where=None):
    """The comparison of the seg modules' judge(): finite, every element inside its bound; returns the largest error / bound."""
    got = (got.detach().double().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float64)).reshape(np.shape(ref))
    ref, bound = np.asarray(ref, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    if where is not None:
        got, ref, bound = got[where], ref[where], bound[where]
    assert np.isfinite(got).all(), f"{name}: non-finite output"
    err = np.abs(got - ref)
    ratio = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    assert (err <= bound).all(), f"{name}: error / bound = {ratio:.3g} at {np.unravel_index((err / np.maximum(bound, 1e-300)).argmax(), err.shape)}"
    return ratio


def report(kernel, case, shape, ratio):
    print(f"SEG-PATHS {kernel} [{case['path']}] {shape}: ratio={ratio:.4g}")
    key = (kernel, case["path"])
    RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)


def bits(t):
    return t.contiguous().view(torch.uint8) if t.dtype != torch.uint8 else t


def same_bits(a, b):
    return all((x is None and y is None) or torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def device_phi(y, B, C):
    from dinox import ops
    return ops.signed_distance_map(torch.from_numpy(np.array(y)).to(DEV), torch.from_numpy(L.SPACING[:B]), C)


def shape_of(c):
    return f"g={c['g']} u={c['u']} B={c['B']} C={c['C']}"


# ------------------------------------------------------------------------------------------ what each kernel's module asserts, per case
def check_loss(name, loss, stats, nv, dz):
    _, fwd, ref_dz, e_dz = L.loss_oracle(name)
    assert nv.cpu().tolist() == [fwd["nv"], 0]
    assert torch.equal(stats[2].cpu().double(), torch.from_numpy(fwd["stats"][2]))      # the label counts are integers
    f = max(ratio_of("fwd loss", loss, fwd["loss"], fwd["e_loss"]), ratio_of("fwd stats", stats, fwd["stats"], fwd["e_stats"]))
    return f, ratio_of("bwd dz", dz, ref_dz, e_dz)


def check_bd(name, phi, loss, stats, nv, dz):
    fwd, ref_dz, e_dz = L.bd_oracle(name, phi.cpu().numpy())
    assert nv.cpu().tolist() == [fwd["nv"], 0]
    f = max(ratio_of(f"bd fwd {what}", loss[i], fwd["loss"][i:i + 1], fwd["e_loss"][i:i + 1]) for i, what in enumerate(("L", "CE", "Dice", "BD")))
    return max(f, ratio_of("bd fwd stats", stats, fwd["stats"], fwd["e_stats"])), ratio_of("bd bwd dz", dz, ref_dz, e_dz)


def check_predict(name, pred, counts):
    c, z, y = L.loss_inputs(name)
    ref, margin, e_l = SO.predict(z, c["g"], c["u"])
    decided = margin > e_l
    pred = pred.cpu().numpy()
    assert pred.dtype == np.uint8 and pred.shape == ref.shape and (pred < c["C"]).all() and (pred[decided] == ref[decided]).all()
    assert 1.0 - decided.mean() <= 0.01
    counts = counts.cpu().numpy().reshape(-1)              # [3 C] from ops, [3 C + 1] from the entry point: the last one counts bad labels
    assert counts.size == 3 * c["C"] or counts[3 * c["C"]] == 0
    assert np.array_equal(counts[:3 * c["C"]].reshape(3, c["C"]), SO.counts(pred, y, c["C"]))


def check_calib(name, pred, conf, ent, hist, tail, sums):
    """The comparisons of tests/test_segcalib_gpu.py::one_case."""
    c, z, y = L.loss_inputs(name)
    cal, o = L.calib_oracle(name)
    pred, conf, ent = pred.cpu().numpy(), conf.cpu().numpy(), ent.cpu().numpy()
    assert 1.0 - cal.decided.mean() <= 0.01
    assert (pred[cal.decided] == cal.pred[cal.decided]).all()
    r = max(ratio_of("conf", conf, o["conf"], o["e_conf"], cal.decided), ratio_of("entropy", ent, o["entropy"], o["e_entropy"]))
    assert ((conf >= 0) & (conf <= 1)).all() and ((ent >= 0) & (ent <= 1)).all()
    want_hist, want_tail = CO.histogram(pred, conf, y, c["C"], c["NB"])        # from the kernel's own maps: integer for integer
    assert hist.dtype == torch.int64 and np.array_equal(hist.cpu().numpy().reshape(c["NB"], 3), want_hist)
    assert np.array_equal(tail.cpu().numpy(), want_tail) and want_tail.tolist() == [o["nv"], 0, 0]
    s = sums.cpu().numpy()
    return max([r] + [ratio_of(f"sum {k}", s[i:i + 1], o["sums"][i:i + 1], o["e_sums"][i:i + 1]) for i, k in enumerate(CO.NAMES)])


# ------------------------------------------------------------------------------------------ loss, prediction, calibration: through ops
@pytest.mark.parametrize("case", P.LOSS_CASES, ids=lambda c: c["name"])
def test_loss_predict_and_calib(case):
    from dinox import ops
    name = case["name"]
    c, z, y = L.loss_inputs(name)
    g, u, B, C, c0, s, NB = c["g"], c["u"], c["B"], c["C"], c["c0"], c["s"], c["NB"]
    zt, yt = on_device(np.array(z), c["zoff"]), torch.from_numpy(np.array(y)).to(DEV)
    w_ce, w_dice = c["weights"]

    def plain():
        loss, stats, saved = ops.seg_loss_fwd(zt, yt, w_ce, w_dice, c0)
        return loss, stats, saved[3], ops.seg_loss_bwd(saved, 1.0)

    a = plain()
    f, b = check_loss(name, *a)
    assert same_bits(a, plain()), "a second call of the loss pair gives other bits"
    report("seg_loss_fwd", c, shape_of(c), f)
    report("seg_loss_bwd", c, shape_of(c), b)

    # the boundary pair, phi from ops as tests/test_bdloss_gpu.py builds it
    phi = device_phi(y, B, C)
    t_ce, t_dice, t_bd = c["triple"]

    def boundary(w1, w2, w3):
        loss, stats, saved = ops.seg_loss_bd_fwd(zt, yt, phi, w1, w2, w3, c0)
        return loss, stats, saved[4], ops.seg_loss_bd_bwd(saved, 1.0)

    d = boundary(t_ce, t_dice, t_bd)
    f, b = check_bd(name, phi, *d)
    assert same_bits(d, boundary(t_ce, t_dice, t_bd)), "a second call of the boundary pair gives other bits"
    report("seg_loss_bd_fwd", c, shape_of(c), f)
    report("seg_loss_bd_bwd", c, shape_of(c), b)
    zero = boundary(w_ce, w_dice, 0.0)                      # w_bd = 0: the bits of the entry points without the term
    assert same_bits((zero[0][:3], zero[1], zero[2], zero[3]), a), "w_bd = 0 does not reproduce seg_loss_fwd / seg_loss_bwd"

    # all ignored: exactly zero, bit for bit
    ignored = torch.full_like(yt, 255)
    loss, _, saved = ops.seg_loss_fwd(zt, ignored, w_ce, w_dice, c0)
    assert not bits(loss).any() and not bits(ops.seg_loss_bwd(saved, 1.0)).any()
    loss, _, saved = ops.seg_loss_bd_fwd(zt, ignored, phi, t_ce, t_dice, t_bd, c0)
    assert not bits(loss).any() and not bits(ops.seg_loss_bd_bwd(saved, 1.0)).any()

    # prediction
    pred, counts = ops.seg_predict(zt, u, yt)
    check_predict(name, pred, counts)
    assert same_bits((pred, counts), ops.seg_predict(zt, u, yt)) and torch.equal(ops.seg_predict(zt, u), pred)
    report("seg_predict", c, shape_of(c), 0.0)

    # calibration, with labels and without
    def calib():
        return ops.seg_calib(zt, u, yt, inv_temperature=s, bins=NB, want_conf=True, want_entropy=True)

    res = calib()
    assert torch.equal(res.pred, pred), "seg_calib's pred is not seg_predict's"
    r = check_calib(name, *res)
    assert same_bits(res, calib()), "a second call of seg_calib gives other bits"
    bare = ops.seg_calib(zt, u, inv_temperature=s, want_conf=True, want_entropy=True)
    assert bare.hist is None and bare.sums is None and same_bits(bare[:3], res[:3])
    gone = ops.seg_calib(zt, u, ignored, inv_temperature=s, bins=NB)
    assert not bits(gone.sums).any() and not gone.hist.any() and torch.equal(gone.pred, pred)
    report("seg_calib", c, shape_of(c), r)

    # T = 0 of the refinement: seg_predict's map and counts, seg_calib's confidence
    gt = on_device(make_guide(np.random.default_rng([79, c["i"]]), B, g * u), 1 - c["zoff"])
    p0, c0_, n0 = ops.seg_refine(zt, gt, u, yt, iters=0, radius=1, dilation=1, inv_temperature=s, want_conf=True)
    assert torch.equal(p0, pred) and torch.equal(n0, counts) and torch.equal(bits(c0_), bits(res.conf)), "T = 0 is not seg_predict / seg_calib"


# ------------------------------------------------------------------------------------------ offset pointers: the C entry points
def guarded_bytes(n, off, fill):
    """n bytes on the device, ``off`` bytes past a 4-byte boundary, with at least 64 bytes of ``fill`` on either side."""
    buf = torch.full((n + 136,), fill, dtype=torch.uint8, device=DEV)
    start = (-buf.data_ptr()) % 4 + 64 + off
    view = buf[start:start + n]
    assert view.data_ptr() % 4 == off and start >= 64 and start + n + 64 <= buf.numel()
    return buf, start, view


def guards_intact(buf, start, n, fill):
    return bool((buf[:start] == fill).all()) and bool((buf[start + n:] == fill).all())


def raw_run(name, yoff, poff):
    """Every label- or prediction-touching entry point of the loss family on explicit pointers: the labels ``yoff`` and both prediction
    maps ``poff`` bytes past a 4-byte boundary.  -> the outputs, the label and prediction guards checked."""
    from dinox import _lib, ops
    lib, check, st = _lib.lib, _lib.check, ops._stream()
    c, z, y = L.loss_inputs(name)
    g, u, B, C, c0, s, NB = c["g"], c["u"], c["B"], c["C"], c["c0"], c["s"], c["NB"]
    assert P.wide(yoff, u) == (yoff == 0) and P.wide(poff, u) == (poff == 0)
    n = y.size
    zt = on_device(np.array(z), c["zoff"])
    ybuf, ys, yv = guarded_bytes(n, yoff, 255)
    yv.copy_(torch.from_numpy(np.array(y)).reshape(-1))
    w_ce, w_dice = c["weights"]
    t_ce, t_dice, t_bd = c["triple"]
    f32 = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)
    i64 = lambda k: torch.full((k,), -1, dtype=torch.int64, device=DEV)
    out = {}
    # the plain pair
    loss, stats, nv, dz = f32(3), f32(3, C), i64(2), f32(*z.shape)
    ws = f32(int(lib.dinox_seg_loss_bd_ws_bytes(B, g, u, C)) // 4)
    assert 0 < lib.dinox_seg_loss_ws_bytes(B, g, u, C) <= 4 * ws.numel()
    check(lib.dinox_seg_loss_fwd(zt.data_ptr(), yv.data_ptr(), loss.data_ptr(), stats.data_ptr(), nv.data_ptr(), ws.data_ptr(), B, g, u, C, c0, w_ce,
                                 w_dice, st), "dinox_seg_loss_fwd")
    check(lib.dinox_seg_loss_bwd(zt.data_ptr(), yv.data_ptr(), stats.data_ptr(), nv.data_ptr(), dz.data_ptr(), ws.data_ptr(), B, g, u, C, c0, w_ce,
                                 w_dice, 1.0, st), "dinox_seg_loss_bwd")
    out["plain"] = (loss, stats, nv, dz)
    # the boundary pair
    phi = device_phi(y, B, C)
    bl, bstats, bnv, bdz = f32(4), f32(3, C), i64(2), f32(*z.shape)
    check(lib.dinox_seg_loss_bd_fwd(zt.data_ptr(), yv.data_ptr(), phi.data_ptr(), bl.data_ptr(), bstats.data_ptr(), bnv.data_ptr(), ws.data_ptr(), B, g,
                                    u, C, c0, t_ce, t_dice, t_bd, st), "dinox_seg_loss_bd_fwd")
    check(lib.dinox_seg_loss_bd_bwd(zt.data_ptr(), yv.data_ptr(), phi.data_ptr(), bstats.data_ptr(), bnv.data_ptr(), bdz.data_ptr(), ws.data_ptr(), B, g,
                                    u, C, c0, t_ce, t_dice, t_bd, 1.0, st), "dinox_seg_loss_bd_bwd")
    out["bd"] = (bl, bstats, bnv, bdz)
    out["phi"] = phi
    # prediction
    pbuf, ps, pv = guarded_bytes(n, poff, CANARY)
    counts = i64(3 * C + 1)
    check(lib.dinox_seg_predict(zt.data_ptr(), yv.data_ptr(), pv.data_ptr(), counts.data_ptr(), B, g, u, C, st), "dinox_seg_predict")
    out["predict"] = (pv.reshape(B, g * u, g * u), counts)
    # calibration
    qbuf, qs, qv = guarded_bytes(n, poff, CANARY)
    conf, ent, hist, sums = f32(B, g * u, g * u), f32(B, g * u, g * u), i64(3 * NB + 3), f32(5)
    cws = f32(int(lib.dinox_seg_calib_ws_bytes(B, g, u, C, NB)) // 4)
    check(lib.dinox_seg_calib(zt.data_ptr(), yv.data_ptr(), s, qv.data_ptr(), conf.data_ptr(), ent.data_ptr(), hist.data_ptr(), sums.data_ptr(),
                              cws.data_ptr(), B, g, u, C, NB, st), "dinox_seg_calib")
    out["calib"] = (qv.reshape(B, g * u, g * u), conf, ent, hist[:3 * NB], hist[3 * NB:], sums)
    torch.cuda.synchronize()
    # the packed store writes four bytes at a time: a group that straddled a cell's edge or the map's end would show in the canary
    assert guards_intact(pbuf, ps, n, CANARY) and guards_intact(qbuf, qs, n, CANARY), "a prediction store left its map"
    assert guards_intact(ybuf, ys, n, 255) and torch.equal(yv.cpu(), torch.from_numpy(np.array(y)).reshape(-1))
    return out


@pytest.mark.parametrize("u", P.ACCESS_FACTORS)
def test_wide_and_byte_access_agree(u):
    """The two access cases of a factor: the 32-bit label load with the packed store, the byte load with the byte store.  Each is held to
    the oracles; the two give the same bits in every output (the labels and the logits are the same, only the pointers moved)."""
    from dinox import ops
    wide_case, byte_case = (c for c in P.ACCESS_CASES if c["u"] == u)
    assert (wide_case["yoff"], wide_case["poff"]) == (0, 0) and byte_case["yoff"] in (1, 3) and byte_case["poff"] == 2
    name = wide_case["of"]
    lc = P.BY_NAME["loss", name]
    runs = []
    for c in (wide_case, byte_case):
        out = raw_run(name, c["yoff"], c["poff"])
        f, b = check_loss(name, *out["plain"])
        fb, bb = check_bd(name, out["phi"], *out["bd"])
        check_predict(name, *out["predict"])
        r = check_calib(name, *out["calib"])
        assert torch.equal(out["calib"][0], out["predict"][0])
        for kernel, ratio in (("seg_loss_fwd", f), ("seg_loss_bwd", b), ("seg_loss_bd_fwd", fb), ("seg_loss_bd_bwd", bb), ("seg_predict", 0.0),
                              ("seg_calib", r)):
            report(kernel, c, f"{shape_of(lc)} labels+{c['yoff']} pred+{c['poff']}", ratio)
        runs.append(out)
    for k in ("plain", "bd", "predict", "calib"):
        assert same_bits(runs[0][k], runs[1][k]), f"{k}: the byte paths give other bits than the wide ones"
    zt = on_device(np.array(L.loss_inputs(name)[1]), lc["zoff"])
    assert torch.equal(ops.seg_predict(zt, u), runs[1]["predict"][0])


# ------------------------------------------------------------------------------------------ refinement: every (CP, r)
@pytest.mark.parametrize("case", P.REFINE_CASES, ids=lambda c: c["name"])
def test_refine_iteration_kernel(case):
    """The comparisons of tests/test_segrefine_gpu.py::one_case, once with labels and counts and once without."""
    from dinox import ops
    c, z, guide, y = L.refine_inputs(case["name"])
    o = L.refine_oracle(case["name"])
    p, i = c["params"], c["i"]
    kw = dict(iters=p["T"], radius=p["r"], dilation=p["d"], sigma_xy=p["sigma_xy"], sigma_i=p["sigma_i"], mix=p["lam"], weight=p["w"],
              inv_temperature=p["s"])
    zt, gt, yt = on_device(z, i % 2), on_device(guide, (i // 2) % 2), torch.from_numpy(y).to(DEV)
    pred, conf, counts = ops.seg_refine(zt, gt, c["u"], yt, want_conf=True, **kw)
    pred_h, conf_h = pred.cpu().numpy(), conf.cpu().numpy()
    assert pred.dtype == torch.uint8 and conf.dtype == torch.float32 and counts.dtype == torch.int64 and tuple(counts.shape) == (3, c["C"])
    assert ((conf_h >= 0) & (conf_h <= 1)).all() and (pred_h < c["C"]).all()
    assert np.array_equal(counts.cpu().numpy(), SO.counts(pred_h, y, c["C"])), "counts differ from the recount of the returned map"
    dec = o["decided"]
    assert 1.0 - dec.mean() <= 0.01
    assert (pred_h[dec] == o["pred"][dec]).all(), f"{(pred_h[dec] != o['pred'][dec]).sum()} decided pixels differ from the float64 arg-max"
    r = ratio_of("conf", conf_h, o["conf"], o["e_conf"], dec)
    bare = ops.seg_refine(zt, gt, c["u"], **kw)
    assert bare[1] is None and bare[2] is None and torch.equal(bare[0], pred)
    assert same_bits((pred, conf, counts), ops.seg_refine(zt, gt, c["u"], yt, want_conf=True, **kw)), "a second call gives other bits"
    report("seg_refine", c, f"{shape_of(c)} r={p['r']} d={p['d']} T={p['T']}", r)


# ------------------------------------------------------------------------------------------ blend
@pytest.mark.parametrize("case", P.BLEND_CASES, ids=lambda c: c["name"])
def test_blend_kernel(case):
    """The comparisons of tests/test_segblend_gpu.py::test_blend_equals_the_oracle."""
    from dinox import ops
    c, (H, W, t, g), ys, xs, win, z, want = L.blend_case(case["name"])
    rng = np.random.default_rng(c["seed"] + 7)
    lab = rng.integers(0, c["C"], size=(c["B"], H, W)).astype(np.uint8)
    lab[rng.random(lab.shape) < 0.1] = 255
    zt, lt = torch.from_numpy(np.array(z)).to(DEV), torch.from_numpy(lab).to(DEV)
    args = (ys, xs, c["flips"], win, H, W, t)
    pred, counts, conf = ops.seg_blend_predict(zt, *args, labels=lt, want_conf=True)
    assert pred.dtype == torch.uint8 and conf.dtype == torch.float32 and counts.dtype == torch.int64 and tuple(counts.shape) == (3, c["C"])
    share, worst = want.check(pred.cpu().numpy(), conf.cpu().numpy())
    assert np.array_equal(counts.cpu().numpy(), BLO.confusion_counts(pred.cpu().numpy(), lab, c["C"]))
    assert torch.equal(ops.seg_blend_predict(zt, *args), pred)
    assert same_bits((pred, counts, conf), ops.seg_blend_predict(zt, *args, labels=lt, want_conf=True)), "a second call gives other bits"
    report("seg_blend_predict", c, f"{H}x{W} t={t} g={g} B={c['B']} F={c['F']} C={c['C']} exempt={share:.1e}", worst)


def test_zz_report_path_maxima():
    """Not a check of its own: the largest error / bound per kernel and path (each was asserted <= 1 above)."""
    for kernel, path in sorted(RATIOS):
        print(f"SEG-PATHS max {kernel:20s} {path:64s} {RATIOS[kernel, path]:.4f}")
