#!/usr/bin/env python3
"""Bit-level fingerprint of every kernel that runs the LayerNorm row arithmetic of csrc/ln_row.h.

    DINOX_LIB=/path/to/other/libdinox_hip.so python tools/ln_row_ab.py > a.txt
    python tools/ln_row_ab.py > b.txt && diff a.txt b.txt

Calls the C ABI directly (dinox._lib.lib) on fixed seeded inputs -- the hostile x and dy families of oracle/ln_bounds.py, taken in
turn -- and prints one SHA-256 per output array.  One library per process (DINOX_LIB chooses it); every call is synchronised and its
return code checked, and the first error ends the run.  Two builds compute the same bits iff their outputs are the same text."""
import hashlib
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dino-x_amd")]
import numpy as np
import torch

from dinox import _lib
from oracle import ln_bounds as LB

L, DEV, EPS, F32, BF16 = _lib.lib, "cuda", 1e-5, 0, 1
_xf, _dyf = itertools.cycle(LB.X_FAMILIES), itertools.cycle(LB.DY_FAMILIES)


def dev(a, bf16=False, off=0):
    """Array on the device (as bf16 if asked), `off` bytes past a 16-byte boundary."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    t = t.bfloat16() if bf16 else t
    pad = off // t.element_size()
    buf = torch.empty(t.numel() + pad, dtype=t.dtype, device=DEV)
    buf[pad:].copy_(t.reshape(-1))
    return buf[pad:].view(t.shape)


def empty(shape, dt=torch.float32, off=0):
    pad = off // torch.empty(0, dtype=dt).element_size()
    n = int(np.prod(shape))
    return torch.full((n + pad,), 7, dtype=dt, device=DEV)[pad:].view(shape)


def ptr(t):
    return None if t is None else t.data_ptr()


def call(name, *args):
    _lib.check(getattr(L, name)(*args, None), name)
    torch.cuda.synchronize()


def show(tag, **outs):
    for k, t in outs.items():
        raw = t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else t.dtype).cpu().numpy().tobytes()
        print(f"{tag} {k} {hashlib.sha256(raw).hexdigest()}", flush=True)


def stats(x):
    x64 = x.astype(np.float64)
    mu = x64.mean(1)
    return mu.astype(np.float32), (1 / np.sqrt(((x64 - mu[:, None]) ** 2).mean(1) + EPS)).astype(np.float32)


def layernorm(rows, dim, off):
    xfam, dyfam = next(_xf), next(_dyf)
    x_h = LB.make_x(xfam, rows, dim)
    gam_h, bet_h = LB.make_params(dim)
    mu_h, rs_h = stats(x_h)
    x, gam, bet, mu, rs = dev(x_h, off=off), dev(gam_h, off=off), dev(bet_h, off=off), dev(mu_h), dev(rs_h)
    tag = f"ln rows={rows} dim={dim} off={off} x={xfam}"
    for odt in (F32, BF16):
        y, m, r = empty((rows, dim), torch.bfloat16 if odt else torch.float32, off), empty(rows), empty(rows)
        call("dinox_layernorm_fwd", ptr(x), ptr(gam), ptr(bet), ptr(y), ptr(m), ptr(r), rows, dim, EPS, odt)
        show(f"{tag} fwd out={odt}", y=y, mean=m, rstd=r)
    ws = empty(L.dinox_layernorm_bwd_ws_bytes(rows, dim) // 4)
    add_h = LB.make_x("randn", rows, dim, seed=1)
    seed_w, seed_b = LB.make_params(dim, seed=2)
    for ddt, has_add, lowp, acc in itertools.product((F32, BF16), (0, 1), (0, 1), (0, 1)):
        dy = dev(LB.make_dy(dyfam, x_h, gam_h, EPS, bf16=bool(ddt)), bf16=bool(ddt), off=off)
        dx, add = empty((rows, dim), off=off), dev(add_h, off=off) if has_add else None
        lp = empty((rows, dim), torch.bfloat16, off) if lowp else None
        dw, db = dev(seed_w), dev(seed_b)
        call("dinox_layernorm_bwd", ptr(dy), ptr(x), ptr(gam), ptr(mu), ptr(rs), ptr(dx), ptr(add), ptr(lp), ptr(dw), ptr(db), ptr(ws),
             rows, dim, ddt, acc)
        outs = dict(dx=dx, dw=dw, db=db, **({"dx_lowp": lp} if lowp else {}))
        show(f"{tag} bwd dy={dyfam}/{ddt} add={has_add} lowp={lowp} acc={acc}", **outs)


def linear(M, K):
    N = 384
    xfam, dyfam = next(_xf), next(_dyf)
    r = np.random.default_rng([17, M, K])
    a = dev(0.5 * r.standard_normal((M, K), dtype=np.float32), bf16=True)
    w = dev((2.0 / np.sqrt(K)) * r.standard_normal((N, K), dtype=np.float32), bf16=True)
    bias = dev(0.1 * r.standard_normal(N, dtype=np.float32))
    gam_h, bet_h = LB.make_params(N)
    gam, bet = dev(gam_h), dev(bet_h)
    x_h = LB.make_x(xfam, M, N)
    tag = f"linear M={M} K={K} x={xfam}"
    assert L.dinox_linear_residual_ln_ok(M, N, K) == 1 and L.dinox_linear_ln_bwd_ok(M, N, K) == 1, tag
    for has_res, ydt in itertools.product((0, 1), (BF16, F32)):
        res = dev(x_h) if has_res else None
        xo, y, m, s = empty((M, N)), empty((M, N), torch.float32 if ydt == F32 else torch.bfloat16), empty(M), empty(M)
        call("dinox_linear_residual_ln", ptr(a), ptr(w), ptr(bias), ptr(res), ptr(xo), ptr(gam), ptr(bet), EPS, ptr(y), ydt, ptr(m), ptr(s), M, N, K)
        show(f"{tag} residual_ln res={has_res} y={ydt}", x=xo, y=y, mean=m, rstd=s)
    mu_h, rs_h = stats(x_h)
    x, mu, rs = dev(x_h), dev(mu_h), dev(rs_h)
    ws = empty(L.dinox_layernorm_bwd_ws_bytes(M, N) // 4)
    add_h = LB.make_dy(dyfam, x_h, gam_h, EPS)
    for mode, acc in (("none", 0), ("other", 1), ("alias", 0)):
        add = None if mode == "none" else dev(add_h)
        dx = add if mode == "alias" else empty((M, N))
        lp, dw, db = empty((M, N), torch.bfloat16), dev(bet_h), dev(gam_h)
        call("dinox_linear_ln_bwd", ptr(a), ptr(w), ptr(x), ptr(gam), ptr(mu), ptr(rs), ptr(dx), ptr(add), ptr(lp), ptr(dw), ptr(db), ptr(ws), M, N, K, acc)
        show(f"{tag} ln_bwd add={mode}/{dyfam} acc={acc}", dx=dx, dx_lowp=lp, dgamma=dw, dbeta=db)


def tokens():
    V, P, R, D = 3, 16, 4, 384
    r = np.random.default_rng(19)
    f = lambda *s: r.standard_normal(s, dtype=np.float32)
    patches, cls, pos, regs, scale = dev(f(V, P, D), bf16=True), dev(f(D)), dev(f(1 + P, D)), dev(f(R, D)), dev(f(V, D))
    tok = empty((V, 1 + P + R, D))
    call("dinox_tokens_fwd", ptr(patches), ptr(cls), ptr(pos), ptr(regs), ptr(scale), ptr(tok), V, P, R, D, BF16)
    show("tokens fwd", tokens=tok)
    dt = dev(f(V, 1 + P + R, D))
    dp, dc, dpos, dr, ds = empty((V, P, D), torch.bfloat16), empty(D), empty((1 + P, D)), empty((R, D)), empty((V, D))
    call("dinox_tokens_bwd", ptr(dt), ptr(dp), ptr(dc), ptr(dpos), ptr(dr), ptr(ds), V, P, R, D, BF16)
    show("tokens bwd", dpatches=dp, dcls=dc, dpos=dpos, dregs=dr, dscale=ds)


def main():
    assert L.dinox_device_ok() == 1, _lib.last_error()
    print(f"# library: {os.path.basename(os.path.dirname(_lib.LIB_PATH))}/{os.path.basename(_lib.LIB_PATH)}", file=sys.stderr)
    for (dim, off), rows in itertools.product([(384, 0), (64, 0), (512, 0), (1024, 0), (2048, 0), (30, 0), (384, 4)], (1, 5, 33, 1030)):
        layernorm(rows, dim, off)
    for K, M in itertools.product((384, 1536), (1, 207, 208, 209, 417)):
        linear(M, K)
    tokens()


if __name__ == "__main__":
    main()
