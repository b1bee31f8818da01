"""The elementwise attention bounds of oracle/attention_bounds.py, checked without a GPU against a tile-by-tile torch emulation of
the arithmetic the attention kernels document (32-key / 32-query tiles, online softmax in the log2 domain, P and dS rounded to bf16
before their products, fp32 accumulation, bf16 outputs; the fp32 variant rounds nothing):

  * the fault-free emulation stays at or below 0.75 x every bound, for every input family;
  * four seeded faults of the kind these kernels can have each exceed a bound in a NAMED family;
  * the randn family does NOT catch the skipped output rescale: why the other families exist.
"""
import math

import pytest
import torch

from oracle import attention_bounds as AB

LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
TILE = 32
SHAPES = [(1, 201, 2, 64), (1, 333, 1, 128), (1, 609, 1, 88), (1, 33, 1, 64), (1, 290, 1, 40)]


def _lowp(fp32):
    return (lambda x: x) if fp32 else (lambda x: x.bfloat16().float())


def emulate_fwd(qkv, heads, fp32=False, fault=None):
    """Online-softmax forward over 32-key tiles.  The ragged last tile is padded by re-reading the last valid row (as the LDS-DMA images
    of the whole-strip kernels do) and masked.  Faults: "nomask" (the padded keys count), "norescale" (the output block keeps its old
    scale when the maximum moves in the last tile).  Returns o [B, N, heads d] in the compute dtype and lse [B, heads, N] fp32."""
    q, k, v = (x.float() for x in AB.split_qkv(qkv, heads))
    B, h, N, d = q.shape
    lowp = _lowp(fp32)
    c2 = torch.tensor(1.0 / math.sqrt(d), dtype=torch.float32) * LOG2E
    m = torch.full((B, h, N), -math.inf)
    l = torch.zeros(B, h, N)
    acc = torch.zeros(B, h, N, d)
    for k0 in range(0, N, TILE):
        nv = min(TILE, N - k0)
        rows = torch.arange(k0, k0 + TILE).clamp_max(N - 1)
        s = (q @ k[:, :, rows].transpose(-1, -2)) * c2
        if nv < TILE and fault != "nomask":
            s[..., nv:] = -math.inf
        mn = torch.maximum(m, s.amax(-1))
        alpha = torch.exp2(m - mn)
        p = torch.exp2(s - mn[..., None])
        l = l * alpha + p.sum(-1)
        if not (fault == "norescale" and k0 + TILE >= N):
            acc = acc * alpha[..., None]
        acc = acc + lowp(p) @ v[:, :, rows]
        m = mn
    o = acc / l[..., None]
    o = o.permute(0, 2, 1, 3).reshape(B, N, h * d)
    return (o if fp32 else o.bfloat16()), m * LN2 + torch.log(l)


def emulate_bwd(do, qkv, o, lse, heads, fp32=False, fault=None):
    """dQ over 32-key tiles, dK / dV over 32-query tiles, from the forward's own o and lse.  Faults: "skip_last_q" (the last query tile
    never reaches dK / dV), "delta_row" (delta taken from the neighbouring row).  Returns the packed dqkv in the compute dtype."""
    q, k, v = (x.float() for x in AB.split_qkv(qkv, heads))
    dO, of = AB.heads_first(do, heads).float(), AB.heads_first(o, heads).float()
    B, h, N, d = q.shape
    lowp = _lowp(fp32)
    sc = torch.tensor(1.0 / math.sqrt(d), dtype=torch.float32)
    c2 = sc * LOG2E
    delta = (dO * of).sum(-1, keepdim=True)
    if fault == "delta_row":
        delta = delta.roll(1, dims=-2)
    L2 = (lse.float() * LOG2E)[..., None]
    dq, dk, dv = torch.zeros_like(q), torch.zeros_like(q), torch.zeros_like(q)
    for k0 in range(0, N, TILE):
        kt, vt = k[:, :, k0:k0 + TILE], v[:, :, k0:k0 + TILE]
        p = torch.exp2((q @ kt.transpose(-1, -2)) * c2 - L2)
        ds = p * (dO @ vt.transpose(-1, -2) - delta) * sc
        dq = dq + lowp(ds) @ kt
    for q0 in range(0, N, TILE):
        if fault == "skip_last_q" and q0 + TILE >= N:
            break
        qt, dot = q[:, :, q0:q0 + TILE], dO[:, :, q0:q0 + TILE]
        p = torch.exp2((qt @ k.transpose(-1, -2)) * c2 - L2[:, :, q0:q0 + TILE])
        ds = p * (dot @ v.transpose(-1, -2) - delta[:, :, q0:q0 + TILE]) * sc
        dv = dv + lowp(p).transpose(-1, -2) @ dot
        dk = dk + lowp(ds).transpose(-1, -2) @ qt
    out = torch.stack([dq, dk, dv], 0).permute(1, 3, 0, 2, 4).reshape(B, N, 3 * h * d)
    return out if fp32 else out.bfloat16()


def ratios(case, shape, fp32=False, fwd_fault=None, bwd_fault=None):
    """err / bound of the emulation for o, lse, dq, dk, dv (the backward always runs from a fault-free forward)."""
    B, N, h, d = shape
    dt = torch.float32 if fp32 else torch.bfloat16
    qkv = AB.make_qkv(case, B, N, h, d, seed=N + d, dtype=dt)
    do = AB.make_do(B, N, h, d, seed=N + d, dtype=dt)
    fb = AB.forward_bounds(qkv, h, fp32)
    o, lse = emulate_fwd(qkv, h, fp32, fwd_fault)
    out = {"o": AB.ratio(AB.heads_first(o, h), fb["o"], fb["o_bound"])[0], "lse": AB.ratio(lse, fb["lse"], fb["lse_bound"])[0]}
    if fwd_fault is None:
        bb = AB.backward_bounds(do, qkv, o, lse, h, fp32)
        dq, dk, dv = AB.split_dqkv(emulate_bwd(do, qkv, o, lse, h, fp32, bwd_fault), h)
        for n, g in (("dq", dq), ("dk", dk), ("dv", dv)):
            out[n] = AB.ratio(g, bb[n], bb[n + "_bound"])[0]
    return out


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("case", AB.FAMILIES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_emulation_stays_within_three_quarters_of_every_bound(shape, case, mode):
    r = ratios(case, shape, fp32=mode == "fp32")
    print(f"BOUNDS-CPU {mode} {case} {shape}: " + " ".join(f"{k}={v:.3f}" for k, v in r.items()))
    for k, v in r.items():
        assert v <= 0.75, f"{mode} {case} {shape}: {k} at {v:.3f} x its bound"


# (fault, shape, the family that must catch it, the output it shows in)
FAULTS = [
    ("nomask", (1, 33, 1, 64), "lastkey", "lse"),            # the one valid key of the last tile, counted 32 times: lse off by log 32
    ("nomask", (1, 33, 1, 64), "randn", "o"),                # ... and its value row weighs 32 / 64 instead of 1 / 33
    ("norescale", (1, 609, 1, 88), "ramp", "o"),             # the maximum still rises in the last tile
    ("norescale", (1, 201, 2, 64), "ramp", "o"),
    ("skip_last_q", (1, 201, 2, 64), "fall", "dk"),          # queries 192..200 missing from dK and dV
    ("skip_last_q", (1, 201, 2, 64), "fall", "dv"),
    ("skip_last_q", (1, 33, 1, 64), "onehot", "dv"),         # query 32 is the only one that looks at key (7 * 32 + 3) % 33
    ("delta_row", (1, 201, 2, 64), "ramp", "dq"),            # delta of row i - 1
    ("delta_row", (1, 201, 2, 64), "offset", "dk"),
]


@pytest.mark.parametrize("fault,shape,case,where", FAULTS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_seeded_fault_exceeds_a_bound(fault, shape, case, where):
    fwd = fault in ("nomask", "norescale")
    r = ratios(case, shape, fwd_fault=fault if fwd else None, bwd_fault=None if fwd else fault)
    print(f"FAULT {fault} {case} {shape}: " + " ".join(f"{k}={v:.3g}" for k, v in r.items()))
    assert r[where] > 1.0, f"{fault}: {case} at {shape} does not catch it in {where}: {r}"


def test_randn_misses_the_skipped_rescale():
    """On randn data the row maximum has settled long before the last key tile, so leaving the rescale out there changes nothing the
    bound can see -- and nothing the whole-tensor relative L2 of the older tests can see either.  ramp catches it (above)."""
    shape = (1, 609, 1, 88)
    clean, faulty = ratios("randn", shape), ratios("randn", shape, fwd_fault="norescale")
    assert faulty["o"] <= 1.0 and faulty["lse"] <= 1.0, faulty
    assert ratios("ramp", shape, fwd_fault="norescale")["o"] > 10.0
    print(f"randn, skipped rescale: o at {faulty['o']:.3f} x the bound (fault-free {clean['o']:.3f})")


def test_lse_bound_detects_one_dropped_key_of_a_uniform_row():
    """The lse bound is below 1 / (2N) at every tested N, so log(N) and log(N - 1) are told apart."""
    for N in (19, 201, 609):
        qkv = torch.zeros(1, N, 3 * 64, dtype=torch.bfloat16)
        fb = AB.forward_bounds(qkv, 1)
        dropped = torch.full_like(fb["lse"], math.log(N - 1))
        assert AB.ratio(dropped, fb["lse"], fb["lse_bound"])[0] > 1.0


def test_check_reports_the_index():
    ref = torch.zeros(2, 3, 5, 4, dtype=torch.float64)
    got = ref.clone()
    got[1, 2, 4, 3] = 2.0
    with pytest.raises(AssertionError, match=r"\(1, 2, 4, 3\)"):
        AB.check(got, ref, torch.ones_like(ref), "o")
    got[1, 2, 4, 3] = float("nan")
    with pytest.raises(AssertionError):
        AB.check(got, ref, torch.ones_like(ref), "o")
    assert AB.check(ref + 0.5, ref, torch.ones_like(ref), "o")[0] == 0.5


@pytest.mark.parametrize("case", AB.FAMILIES)
def test_projected_family_keeps_its_character(case):
    """make_xw: x w^T (what the fused projection + attention kernel computes) has the family's softmax: the row maximum of ramp sits in
    the last key tile, of fall in the first, offset scores are near 70 to 80, lastkey rows give the last key nearly all the mass."""
    B, N, h, d, D = 1, 201, 2, 64, 128
    x, w = AB.make_xw(case, B, N, h, d, D, seed=5)
    qkv = (x.double() @ w.double().t()).bfloat16()
    q, k, _ = AB.split_qkv(qkv, h)
    s = q @ k.transpose(-1, -2) / 8.0
    P = torch.softmax(s, -1)
    if case == "ramp":
        assert bool((s.argmax(-1) >= N - 32).all())
    elif case == "fall":
        assert bool((s.argmax(-1) < 32).all())
    elif case == "offset":
        assert 60.0 < float(s.min()) and float(s.max()) < 90.0
    elif case == "lastkey":
        assert float(P[..., N - 1].min()) > 0.99
    elif case == "onehot":
        assert float(P.amax(-1).min()) > 0.45                  # one key, or two equal ones (tokens i and i + D)
