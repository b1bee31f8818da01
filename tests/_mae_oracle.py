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


def removed_mask(ids_restore, len_keep):
    """A patch is removed when its rank is outside [0, len_keep) (include/dinox.h): an out-of-range rank counts as removed."""
    r = np.asarray(ids_restore).astype(np.int64)
    return (r < 0) | (r >= len_keep)


def clamp_keep(ids_keep, L):
    """ids_keep as the kernels use it: clamped into [0, L)."""
    return np.clip(np.asarray(ids_keep).astype(np.int64), 0, L - 1)


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
            if 0 <= r < len_keep:
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
            xd[v, 1 + p] = e[v, 1 + r] if 0 <= r < Lk else mask_token.reshape(-1)
    return xd + dec_pos[None]


def unshuffle_bwd(g, ids_keep, ids_restore):
    """g [V, 1 + L, D] -> (de [V, 1 + Lk, D], dmask_token [D])."""
    g = np.asarray(g, dtype=np.float64)
    V, _, D = g.shape
    Lk = ids_keep.shape[1]
    de = np.empty((V, 1 + Lk, D))
    de[:, 0] = g[:, 0]
    de[:, 1:] = np.take_along_axis(g[:, 1:], np.asarray(ids_keep, dtype=np.int64)[:, :, None], axis=1)
    return de, (g[:, 1:] * removed_mask(ids_restore, Lk)[:, :, None]).sum((0, 1))


def loss_fwd(pred, x, ids_restore, len_keep, p):
    """pred [V, L, 3 p^2] -> the mean over removed patches of the per-patch mean squared error."""
    d = np.asarray(pred, dtype=np.float64) - patchify(x, p)
    removed = removed_mask(ids_restore, len_keep)
    return float(((d * d).mean(-1) * removed).sum() / removed.sum())


def loss_bwd(pred, x, ids_restore, len_keep, p, gscale=1.0):
    d = np.asarray(pred, dtype=np.float64) - patchify(x, p)
    removed = removed_mask(ids_restore, len_keep)
    return gscale * 2.0 * d * removed[:, :, None] / (d.shape[-1] * removed.sum())


def loss_rows(pred, x, ids_restore, len_keep, p):
    """-> [V, L] float64: the per-patch mean squared error on removed patches, 0 on kept ones (the ``ws`` of dinox_mae_loss_fwd)."""
    d = np.asarray(pred, dtype=np.float64) - patchify(x, p)
    return (d * d).mean(-1) * removed_mask(ids_restore, len_keep)


# ------------------------------------------------------------------------------------------ synthetic cases
def make_case(V, H, W, p, Lk, D, seed):
    """Every operand of the eight entry points for V images of H x W pixels in p x p patches, Lk kept, D features, from one seed: images,
    noise (distinct), the ids of the stable-argsort statement, kept patch rows, cls / pos, e, mask_token, dec_pos, pred and the upstream
    gradients of tokens (gtok) and of the un-shuffle (gxd), all fp32.  H != W, any L = (H/p)(W/p) >= 2 (p = 1, H = 1 gives any L)."""
    r = np.random.default_rng(seed)
    L, K = (H // p) * (W // p), 3 * p * p
    f = lambda *s: r.standard_normal(s).astype(np.float32)
    noise = np.stack([r.permutation(L) for _ in range(V)]).astype(np.float32) / np.float32(L)
    ids_restore, ids_keep = mask_ids(noise, Lk)
    return dict(dims=(V, H, W, p, L, Lk, D, K), imgs=f(V, 3, H, W), noise=noise, ids_restore=ids_restore, ids_keep=ids_keep,
                patches=f(V, Lk, D), cls=f(D), pos=f(1 + L, D), e=f(V, 1 + Lk, D), mask_token=f(D), dec_pos=f(1 + L, D), pred=f(V, L, K),
                gtok=f(V, 1 + Lk, D), gxd=f(V, 1 + L, D))


def bf16_round(a):
    """The round-to-nearest-even bf16 image of fp32 values, widened back to fp32 (NaN stays NaN)."""
    a = np.ascontiguousarray(a, np.float32)
    u = a.view(np.uint32).astype(np.uint64)
    out = (((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)
    return np.where(np.isnan(a), a, out)


# ------------------------------------------------------------------------------------------ a-priori bounds
# u = 2^-24 (fp32 round to nearest); gamma_n = n u / (1 - n u) bounds the relative error of any product of n factors (1 + d), |d| <= u.
# Every bound is on the float64 value of the formula on the fp32 (or exactly widened bf16) operands the kernel was handed.
U = 2.0 ** -24
PRESENT_BAR = 1e-5           # what tests/test_mae_gpu.py asserts (of a row's max-abs, or relative for the loss)
THREADS = 256                # MAE_THREADS
GRID_CAP = 4096              # the cap of grid_1d(total, 256, 4096): more than GRID_CAP * THREADS work items make a workgroup loop


def gamma(n):
    return n * U / (1.0 - n * U)


def block_sum_depth(threads=THREADS):
    """Rounded additions on the longest path of ``block_sum`` (csrc/common.h) for one workgroup of ``threads`` lanes: ``wave_sum`` is
    six ``__shfl_xor`` butterfly levels (offsets 32, 16, 8, 4, 2, 1), one rounded add each; lane 0 of each of the threads / 64 waves
    stores its sum, and every thread then adds ``t = 0.f; t += red[0]; ...; t += red[nw - 1]``: nw adds of which the first (0 + x) is
    exact.  256 threads: 6 + (4 - 1) = 9."""
    return 6 + (threads // 64 - 1)


def loss_vw(p, aligned=True):
    """The vector width dinox_mae_loss_fwd / _bwd take: 4 when 3 p^2 % 4 == 0 and pred (and dpred) are 16-byte aligned, else 1."""
    return 4 if (3 * p * p) % 4 == 0 and aligned else 1


def row_loss_roundings(p, vw):
    """Longest chain of roundings a term of one patch's mean takes in mae_loss_rows_kernel: the subtraction (1), the square (1), the
    thread's chain of ceil(K / (256 VW)) VW adds, block_sum, the division by K.  (An fma for ``acc += d * d`` only removes roundings.
    Strictly the subtraction's factor enters squared; the count follows the kernel's operations, one each.)"""
    K = 3 * p * p
    return 2 + -(-K // (THREADS * vw)) * vw + block_sum_depth() + 1


def loss_roundings(p, vw, rows):
    """row_loss_roundings plus mae_loss_mean_kernel: a chain of ceil(rows / 256) adds, block_sum, one division."""
    return row_loss_roundings(p, vw) + -(-rows // THREADS) + block_sum_depth() + 1


def bound_row_loss(ref_rows, p, vw):
    """All terms are non-negative: relative."""
    return gamma(row_loss_roundings(p, vw)) * np.asarray(ref_rows, np.float64)


def bound_loss(ref, p, vw, rows):
    return gamma(loss_roundings(p, vw, rows)) * abs(float(ref))


def bound_dpred(ref):
    """Three roundings: scale to fp32 on the host, the subtraction, the product."""
    return gamma(3) * np.abs(np.asarray(ref, np.float64))


def tokens_bwd_terms(dtok, ids_restore, len_keep):
    """-> (n [1 + L] samples that contribute to every position, sum |terms| [1 + L, D]) of dpos (row 0 is dcls)."""
    a = np.abs(np.asarray(dtok, dtype=np.float64))
    _, _, mag = tokens_bwd(a, ids_restore, len_keep)
    V = a.shape[0]
    n = np.concatenate([[V], (~removed_mask(ids_restore, len_keep)).sum(0)])
    return n, mag


def bound_dpos(dtok, ids_restore, len_keep):
    """One thread, ascending v: n terms are n - 1 rounded adds (0 + x is exact).  n = 0: bound 0, the row is exactly 0."""
    n, mag = tokens_bwd_terms(dtok, ids_restore, len_keep)
    return gamma(np.maximum(n - 1, 0))[:, None] * mag


def dmask_roundings(ids_restore, len_keep):
    """(most removed patches of any sample - 1) + (V - 1): the per-sample chain in ascending p, then the chain over ascending v."""
    rem = removed_mask(ids_restore, len_keep).sum(1)
    return max(int(rem.max()) - 1, 0) + rem.shape[0] - 1


def dmask_constant(ids_restore, len_keep):
    """gamma of dmask_roundings, held at the present tests' 1e-5 where the worst-case chain constant would exceed it (more than 167
    roundings: the cases with L - Lk = 193 and 299): no bound here is looser than the one it replaces.  Rounding errors of
    independent sign grow like sqrt(n) u (1e-6 at n = 300), so the kernel is expected far inside either."""
    return min(gamma(dmask_roundings(ids_restore, len_keep)), PRESENT_BAR)


def bound_dmask(g, ids_restore, len_keep):
    g = np.abs(np.asarray(g, dtype=np.float64))
    return dmask_constant(ids_restore, len_keep) * (g[:, 1:] * removed_mask(ids_restore, len_keep)[:, :, None]).sum((0, 1))


# ------------------------------------------------------------------------------------------ the shapes of the path-complete tests
MASK_L = [2, 255, 256, 257, 1369, 4096]                       # one trip, the 256 boundary on both sides, 518 / 14 squared, MAE_MAX_L
NOISE_FAMILIES = ["distinct", "levels8", "equal", "descending", "specials"]
UNFOLD_HWP = [(8, 12, 4), (12, 8, 4), (28, 42, 14), (21, 35, 7), (32, 48, 16), (64, 96, 32)]
TOKEN_V = [1, 5]
TOKEN_LLK = [(2, 1), (257, 64), (257, 256), (300, 1)]
TOKEN_D = [1, 6, 8, 260, 258, 1028]                           # 1, 6, 258 scalar (258: two chunks); 8, 260 vector; 1028 vector, two chunks
# K = 147 and 675 scalar (675: three trips; 3 p^2 % 4 == 0 exactly when p is even, so p = 18, K = 972 is a vector case); 588, 768, 972, 3072 vector
LOSS_HWP = [(21, 35, 7), (28, 42, 14), (32, 48, 16), (36, 54, 18), (64, 96, 32), (30, 45, 15)]
LOSS_MEAN_HWP = (80, 80, 4)                                   # V = 3: V L = 1200 > 1024 rows for mae_loss_mean_kernel
# make_case arguments whose work-item totals are just above GRID_CAP * THREADS = 1 048 576 and no multiple of it (a second, partial trip of
# the grid-stride loops): D / 4 = 257 feature groups x 4 x 1024 (tokens_fwd, unshuffle_bwd gather), x 4 x 1023 (tokens_bwd copy), x 4 x 1025
# (unshuffle_fwd); 58 x 95 rows x 768 / 4 column groups = 1 057 920 (gather_unfold).
STRIDE_TOKENS = (4, 1, 1024, 1, 1023, 1028, 4)
STRIDE_UNFOLD = (58, 128, 192, 16, 95, 8, 5)


def mask_lks(L):
    return sorted({1, max(L // 4, 1), L - 1})


def noise_family(name, V, L, seed=0):
    r = np.random.default_rng(seed + L)
    if name == "distinct":
        return np.stack([r.permutation(L) for _ in range(V)]).astype(np.float32) / np.float32(L)
    if name == "levels8":
        return (np.floor(r.uniform(0, 8, (V, L))) / 8).astype(np.float32)
    if name == "equal":
        return np.full((V, L), 0.25, np.float32)
    if name == "descending":
        return np.broadcast_to(np.arange(L, 0, -1, dtype=np.float32), (V, L)).copy()
    assert name == "specials"
    n = (np.floor(r.uniform(0, 8, (V, L))) / 8).astype(np.float32)
    sp = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, np.nan], np.float32)
    m = min(L, len(sp))
    n[0, :m] = sp[:m]
    n[-1, L - m:] = sp[:m][::-1]
    return n
