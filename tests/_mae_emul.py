"""fp32 NumPy emulation of the kernels of csrc/mae.hip in the order their comments state: the index arithmetic as the kernels do it,
per-thread strided chains, then the wave butterfly and the four-wave chain of ``block_sum``.  tests/test_mae_paths_cpu.py holds it to
the bounds of tests/_mae_oracle.py and plants defects in it: ``defect=n`` switches on variant n of DEFECTS (one line each, marked
``# defect n`` below).  An output element a kernel would not write is NaN (ids: SENTINEL), as the device tests initialise theirs.

No fused multiply-add is emulated: ``acc += d * d`` may compile to one, which removes a rounding and stays inside the same bound."""
import numpy as np

import _mae_oracle as MO

F32 = np.float32
SENTINEL = -7777
CAP = MO.GRID_CAP * MO.THREADS        # work items one pass of a capped grid covers

DEFECTS = {
    1: "gx / gy formed with H / p instead of W / p (gather_unfold and the loss target)",
    2: "the second trip of the loss kernels' per-thread loop dropped",
    3: "chunk 1 of dpos / dmask_token not written",
    4: "lead ignored in the pred row address",
    5: "ties in mask_ids broken by the higher index",
    6: "NaN ordered below everything in mask_ids",
    7: "elements past 4096 * 256 work items left unwritten",
    8: "dpred on kept patches left as scale * (pred - target)",
    9: "the VW = 1 tail: the last D % 4 columns dropped",
}


def vw_of(D, aligned=True):
    return 4 if D % 4 == 0 and aligned else 1


def _unwritten(out, vw, defect, D=None):
    """Defects 7 and 9 on an output whose work item idx covers elements [idx vw, idx vw + vw) of the flattened array."""
    out = np.array(out, F32)
    if defect == 7:
        out.reshape(-1)[CAP * vw:] = np.nan                                      # defect 7
    if defect == 9 and vw == 1 and D is not None:
        out.reshape(-1, D)[:, D - D % 4:] = np.nan                               # defect 9
    return out


def order_key(noise, defect=None):
    f = np.asarray(noise, F32)
    u = (f + F32(0.0)).view(np.uint32)
    key = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
    return np.where(np.isnan(f), np.uint32(0 if defect == 6 else 0xffffffff), key)                     # defect 6


def mask_ids(noise, Lk, defect=None):
    key = order_key(noise, defect).astype(np.int64)
    V, L = key.shape
    ids_restore = np.empty((V, L), np.int32)
    ids_keep = np.full((V, Lk), SENTINEL, np.int32)
    q = np.arange(L)
    for v in range(V):
        k = key[v]
        below = (k[None, :] < k[:, None]).sum(1)
        same = k[None, :] == k[:, None]
        tie = (same & ((q[None, :] > q[:, None]) if defect == 5 else (q[None, :] < q[:, None]))).sum(1)  # defect 5
        r = (below + tie).astype(np.int32)
        ids_restore[v] = r
        ids_keep[v, r[r < Lk]] = q[r < Lk]
    return ids_restore, ids_keep


def _pixel(x, v, c, l, py, px, p, defect):
    """x[v][c][gy p + py][gx p + px] for patch l, by the kernels' own index arithmetic (a wrong address is wrapped into the array)."""
    V, _, H, W = x.shape
    g = (H // p) if defect == 1 else (W // p)                                                          # defect 1
    gx, gy = l % g, l // g
    addr = ((v * 3 + c) * H + (gy * p + py)) * W + gx * p + px
    return np.take(x.reshape(-1), addr, mode="wrap")


def gather_unfold(x, ids_keep, p, ld, bf16=False, defect=None, aligned=True):
    x = np.asarray(x, F32)
    V, _, H, W = x.shape
    L, Kd, Lk = (H // p) * (W // p), 3 * p * p, ids_keep.shape[1]
    vw = 4 if p % 4 == 0 and ld % 4 == 0 and aligned else 1
    l = MO.clamp_keep(ids_keep, L).reshape(-1, 1)
    v = np.repeat(np.arange(V), Lk).reshape(-1, 1)
    k = np.arange(Kd)[None, :]
    u = np.zeros((V * Lk, ld), F32)
    u[:, :Kd] = _pixel(x, v, k // (p * p), l, (k // p) % p, k % p, p, defect)
    u = _unwritten(u, vw, defect)
    return MO.bf16_round(u) if bf16 else u


def target(x, p, defect=None):
    """[V, L, 3 p^2] in patchify order j = (py p + px) 3 + c, as mae_stage_target stages it."""
    x = np.asarray(x, F32)
    V, _, H, W = x.shape
    L = (H // p) * (W // p)
    v = np.arange(V).reshape(-1, 1, 1)
    l = np.arange(L).reshape(1, -1, 1)
    j = np.arange(3 * p * p).reshape(1, 1, -1)
    return _pixel(x, v, j % 3, l, (j // 3) // p, (j // 3) % p, p, defect)


def tokens_fwd(patches, cls, pos, ids_keep, aligned=True, defect=None):
    patches, cls, pos = (np.asarray(a, F32) for a in (patches, cls, pos))
    V, Lk, D = patches.shape
    L = pos.shape[0] - 1
    tok = np.empty((V, 1 + Lk, D), F32)
    tok[:, 0] = cls + pos[0]
    tok[:, 1:] = patches + pos[1 + MO.clamp_keep(ids_keep, L)]
    return _unwritten(tok, vw_of(D, aligned), defect, D)


def _chunk1(out, vw, defect):
    if defect == 3:
        out[..., MO.THREADS * vw:] = np.nan                                                            # defect 3
    return out


def tokens_bwd(dtok, ids_restore, Lk, bf16=False, aligned=True, defect=None):
    """-> (dpatches [V, Lk, D], dcls [D], dpos [1 + L, D])."""
    dtok = np.asarray(dtok, F32)
    V, _, D = dtok.shape
    L = ids_restore.shape[1]
    vw = vw_of(D, aligned)
    kept = ~MO.removed_mask(ids_restore, Lk)
    dpos = np.zeros((1 + L, D), F32)
    for v in range(V):                                                     # one thread per (position, feature), ascending v
        dpos[0] = dpos[0] + dtok[v, 0]
        pk = np.nonzero(kept[v])[0]
        dpos[1 + pk] = dpos[1 + pk] + dtok[v, 1 + ids_restore[v, pk]]
    dpos = _unwritten(_chunk1(dpos, vw, defect), vw, 9 if defect == 9 else None, D)
    dpatches = _unwritten(dtok[:, 1:], vw, defect, D)
    return (MO.bf16_round(dpatches) if bf16 else dpatches), dpos[0].copy(), dpos


def unshuffle_fwd(e, mask_token, dec_pos, ids_restore, aligned=True, defect=None):
    e, mask_token, dec_pos = (np.asarray(a, F32) for a in (e, mask_token, dec_pos))
    V, Ne, D = e.shape
    L, Lk = ids_restore.shape[1], Ne - 1
    kept = ~MO.removed_mask(ids_restore, Lk)
    val = np.empty((V, 1 + L, D), F32)
    val[:, 0] = e[:, 0]
    src = np.take_along_axis(e[:, 1:], np.where(kept, ids_restore, 0).astype(np.int64)[:, :, None], axis=1)
    val[:, 1:] = np.where(kept[:, :, None], src, mask_token.reshape(1, 1, -1))
    return _unwritten(val + dec_pos[None], vw_of(D, aligned), defect, D)


def unshuffle_bwd(g, ids_keep, ids_restore, bf16=False, aligned=True, defect=None):
    """-> (de [V, 1 + Lk, D], dmask_token [D], part [V, D])."""
    g = np.asarray(g, F32)
    V, N, D = g.shape
    L, Lk = N - 1, ids_keep.shape[1]
    vw = vw_of(D, aligned)
    rem = MO.removed_mask(ids_restore, Lk)
    part = np.zeros((V, D), F32)
    for p in range(L):                                                     # ascending p, one thread per (sample, feature)
        part[rem[:, p]] = part[rem[:, p]] + g[rem[:, p], 1 + p]
    part = _unwritten(_chunk1(part, vw, defect), vw, 9 if defect == 9 else None, D)
    dmask = np.zeros(D, F32)
    for v in range(V):                                                     # ascending v
        dmask = dmask + part[v]
    de = np.empty((V, 1 + Lk, D), F32)
    de[:, 0] = g[:, 0]
    de[:, 1:] = np.take_along_axis(g[:, 1:], MO.clamp_keep(ids_keep, L)[:, :, None], axis=1)
    de = _unwritten(de, vw, defect, D)
    return (MO.bf16_round(de) if bf16 else de), dmask, part


def block_sum(a):
    """a [..., 256] fp32 -> [...]: six xor-butterfly levels inside each wave of 64, then 0 + red[0] + red[1] + red[2] + red[3]."""
    a = np.array(a, F32)
    lanes = np.arange(a.shape[-1])
    for o in (32, 16, 8, 4, 2, 1):
        a = a + a[..., lanes ^ o]
    t = np.zeros(a.shape[:-1], F32)
    for w in range(a.shape[-1] // 64):
        t = t + a[..., 64 * w]
    return t


def strided_chain(terms, vw=1):
    """terms [..., n] -> [..., 256]: thread t adds groups t, t + 256, ... of vw consecutive terms, in ascending order."""
    terms = np.asarray(terms, F32)
    n = terms.shape[-1]
    trips = -(-n // (MO.THREADS * vw))
    pad = np.zeros(terms.shape[:-1] + (trips * MO.THREADS * vw,), F32)     # (adding +0 to a non-negative or any fp32 sum is exact)
    pad[..., :n] = terms
    pad = pad.reshape(terms.shape[:-1] + (trips, MO.THREADS, vw))
    acc = np.zeros(terms.shape[:-1] + (MO.THREADS,), F32)
    for t in range(trips):
        for i in range(vw):
            acc = acc + pad[..., t, :, i]
    return acc


def _pred_rows(pred, lead, L, defect):
    """The rows the loss kernels address for patch (v, l): [V, L, K] out of pred [V, lead + L, K]."""
    pred = np.asarray(pred, F32)
    V, _, K = pred.shape
    if defect == 4:
        return pred.reshape(-1, K)[:V * L].reshape(V, L, K)                                            # defect 4
    return pred[:, lead:]


def _second_trip(a, vw, defect):
    if defect == 2:
        a = np.array(a, F32)
        a[..., MO.THREADS * vw:2 * MO.THREADS * vw] = 0                                                # defect 2
    return a


def loss_fwd(pred, x, ids_restore, Lk, p, lead=0, aligned=True, defect=None):
    """pred fp32 (a bf16 operand: its widened values) -> (loss fp32, row_loss [V, L] fp32)."""
    V, _, H, W = np.asarray(x).shape
    L, K = (H // p) * (W // p), 3 * p * p
    vw = MO.loss_vw(p, aligned)
    d = _pred_rows(pred, lead, L, defect) - target(x, p, defect)
    acc = strided_chain(_second_trip(d * d, vw, defect), vw)
    rows = (block_sum(acc) / F32(K)).astype(F32)
    rows = np.where(MO.removed_mask(ids_restore, Lk), rows, F32(0)).astype(F32)
    count = F32(V) * F32(L - Lk)
    return F32(block_sum(strided_chain(rows.reshape(-1))) / count), rows


def loss_bwd(pred, x, ids_restore, Lk, p, lead=0, gscale=1.0, bf16_out=False, aligned=True, defect=None):
    V, _, H, W = np.asarray(x).shape
    L, K = (H // p) * (W // p), 3 * p * p
    vw = MO.loss_vw(p, aligned)
    scale = F32(float(F32(gscale)) * 2.0 / (float(K) * float(V) * float(L - Lk)))
    d = (scale * (_pred_rows(pred, lead, L, defect) - target(x, p, defect))).astype(F32)
    if defect == 2:
        d[..., MO.THREADS * vw:2 * MO.THREADS * vw] = np.nan                                            # defect 2
    if defect != 8:                                                                                    # defect 8
        d = np.where(MO.removed_mask(ids_restore, Lk)[:, :, None], d, F32(0)).astype(F32)
    out = np.concatenate([np.zeros((V, lead, K), F32), d], axis=1)
    return MO.bf16_round(out) if bf16_out else out
