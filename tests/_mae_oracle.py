"""float64 NumPy restatement of the five MAE kernels of csrc/mae.hip (mask ids, gather + unfold, tokens, un-shuffle, loss), written from
the formulas in include/dinox.h.  tests/test_mae_cpu.py checks it against fixtures recorded from the reference
(tests/golden/mae_parts.npz); tests/test_mae_gpu.py checks the kernels against both."""
import numpy as np


def mask_ids(noise, len_keep):
    """-> (ids_restore [V, L], ids_keep [V, len_keep]) int32: stable ranks, and the patch of every kept rank."""
    noise = np.asarray(noise)
    V, L = noise.shape
    order = np.argsort(noise, axis=1, kind="stable")
    ids_restore = np.empty((V, L), dtype=np.int32)
    for v in range(V):
        ids_restore[v, order[v]] = np.arange(L, dtype=np.int32)
    return ids_restore, order[:, :len_keep].astype(np.int32)


def unfold(x, p, ld=None):
    """[V,3,H,W] -> [V, L, ld] with column c p p + py p + px (dinox_patch_unfold) and a zero tail."""
    x = np.asarray(x, dtype=np.float64)
    V, _, H, W = x.shape
    u = x.reshape(V, 3, H // p, p, W // p, p).transpose(0, 2, 4, 1, 3, 5).reshape(V, (H // p) * (W // p), 3 * p * p)
    if ld is not None and ld > u.shape[2]:
        u = np.concatenate([u, np.zeros((V, u.shape[1], ld - u.shape[2]))], axis=2)
    return u


def gather_unfold(x, ids_keep, p, ld=None):
    u = unfold(x, p, ld)
    return np.take_along_axis(u, np.asarray(ids_keep, dtype=np.int64)[:, :, None], axis=1).reshape(-1, u.shape[2])


def patchify(x, p):
    """[V,3,H,W] -> [V, L, 3 p^2] with column (py p + px) 3 + c (the loss target)."""
    x = np.asarray(x, dtype=np.float64)
    V, _, H, W = x.shape
    return x.reshape(V, 3, H // p, p, W // p, p).transpose(0, 2, 4, 3, 5, 1).reshape(V, (H // p) * (W // p), 3 * p * p)


def tokens_fwd(patches, cls, pos, ids_keep):
    """patches [V, Lk, D] (kept rows), cls [D], pos [1 + L, D] -> [V, 1 + Lk, D]."""
    patches, cls, pos = (np.asarray(a, dtype=np.float64) for a in (patches, cls, pos))
    V, Lk, D = patches.shape
    tok = np.empty((V, 1 + Lk, D))
    tok[:, 0] = cls.reshape(-1) + pos[0]
    tok[:, 1:] = patches + pos[1 + np.asarray(ids_keep, dtype=np.int64)]
    return tok


def tokens_bwd(dtok, ids_restore, len_keep):
    """-> (dpatches [V, Lk, D], dcls [D], dpos [1 + L, D])."""
    dtok = np.asarray(dtok, dtype=np.float64)
    V, _, D = dtok.shape
    L = ids_restore.shape[1]
    dpos = np.zeros((1 + L, D))
    dpos[0] = dtok[:, 0].sum(0)
    for v in range(V):
        for p in range(L):
            r = int(ids_restore[v, p])
            if r < len_keep:
                dpos[1 + p] += dtok[v, 1 + r]
    return dtok[:, 1:].copy(), dpos[0].copy(), dpos


def unshuffle_fwd(e, mask_token, dec_pos, ids_restore):
    """e [V, 1 + Lk, D], mask_token [D], dec_pos [1 + L, D] -> [V, 1 + L, D]."""
    e, mask_token, dec_pos = (np.asarray(a, dtype=np.float64) for a in (e, mask_token, dec_pos))
    V, Ne, D = e.shape
    L, Lk = ids_restore.shape[1], Ne - 1
    xd = np.empty((V, 1 + L, D))
    xd[:, 0] = e[:, 0]
    for v in range(V):
        for p in range(L):
            r = int(ids_restore[v, p])
            xd[v, 1 + p] = e[v, 1 + r] if r < Lk else mask_token.reshape(-1)
    return xd + dec_pos[None]


def unshuffle_bwd(g, ids_keep, ids_restore):
    """g [V, 1 + L, D] -> (de [V, 1 + Lk, D], dmask_token [D])."""
    g = np.asarray(g, dtype=np.float64)
    V, _, D = g.shape
    Lk = ids_keep.shape[1]
    de = np.empty((V, 1 + Lk, D))
    de[:, 0] = g[:, 0]
    de[:, 1:] = np.take_along_axis(g[:, 1:], np.asarray(ids_keep, dtype=np.int64)[:, :, None], axis=1)
    removed = np.asarray(ids_restore) >= Lk
    return de, (g[:, 1:] * removed[:, :, None]).sum((0, 1))


def loss_fwd(pred, x, ids_restore, len_keep, p):
    """pred [V, L, 3 p^2] -> the mean over removed patches of the per-patch mean squared error."""
    d = np.asarray(pred, dtype=np.float64) - patchify(x, p)
    removed = np.asarray(ids_restore) >= len_keep
    return float(((d * d).mean(-1) * removed).sum() / removed.sum())


def loss_bwd(pred, x, ids_restore, len_keep, p, gscale=1.0):
    d = np.asarray(pred, dtype=np.float64) - patchify(x, p)
    removed = np.asarray(ids_restore) >= len_keep
    return gscale * 2.0 * d * removed[:, :, None] / (d.shape[-1] * removed.sum())
