"""Float64 statements of Sinkhorn-Knopp teacher centring (csrc/sinkhorn.hip) and the fp32 error bounds its tests hold the kernels to.

``sk_literal`` is the loop as DINOv2 publishes it (linear domain: Q = exp(t / tau)^T over its sum; n times: rows of Q -- prototypes --
to sum 1/K, columns -- samples -- to sum 1/B; Q * B), returning Q^T with rows that sum to 1.  ``sk_center`` is the log-domain recurrence
of include/dinox.h,
    a_0 = 0,   b_n[k] = -log sum_i exp(z[i,k] + a_{n-1}[i]),   a_n[i] = -log sum_k exp(z[i,k] + b_n[k]),   centre = -tau b_n,
for which softmax_k((t[i,k] - centre[k]) / tau) is that Q^T (tests/test_sinkhorn_cpu.py proves it).  No project code is called.

The bounds follow tests/_small_kernels_oracle.py: (n_ops + 2) u S for the rounded operations, plus the project's existing tolerance for
expf / logf (CE_LOSS_RTOL).  No new constant."""
import numpy as np

from _small_kernels_oracle import CE_DS_RTOL, CE_LOSS_RTOL, F64, TINY, U, block_adds, dino_inputs, f32  # noqa: F401  (re-exported to the tests)

CHUNK = 32          # rows of one column-pass workgroup (SK_CHUNK in csrc/sinkhorn.hip)


# ------------------------------------------------------------------------------------------ the two statements
def sk_literal(t, tt, iters, dt=F64):
    """The DINOv2 loop, linear domain.  t [R,K] teacher logits, tt the teacher temperature (its fp32 value, as the C ABI receives it).
    ``dt=np.longdouble`` keeps the same loop finite where exp(t / tt) leaves float64 (|t / tt| > 709): same statements, wider exponent."""
    t = np.asarray(t, dt)
    B, K = t.shape
    Q = np.exp(t / dt(f32(tt))).T                  # [K, B]
    Q = Q / Q.sum()
    for _ in range(iters):
        Q = Q / Q.sum(axis=1, keepdims=True)       # every prototype: total weight 1 ...
        Q = Q / dt(K)                              # ... / K
        Q = Q / Q.sum(axis=0, keepdims=True)       # every sample: total weight 1 ...
        Q = Q / dt(B)                              # ... / B
    Q = Q * dt(B)                                  # columns sum to 1: one assignment per sample
    return Q.T


def _lse(x, axis):
    m = x.max(axis, keepdims=True)
    e = np.exp(x - m)
    s = e.sum(axis, keepdims=True)
    return (m + np.log(s)).squeeze(axis), m, e, s


def col_pass(t, a, inv, dt=F64):
    """lse over the rows: out[k] = log sum_i exp(t[i,k] inv + a[i]).  -> (lse [K], parts for the bound)."""
    t = np.asarray(t, dt)
    x = t * dt(inv) + (dt(0) if a is None else np.asarray(a, dt)[:, None])
    lse, m, e, s = _lse(x, 0)
    return lse, {"x": x, "z": t * dt(inv), "m": m, "e": e, "s": s, "lse": lse, "axis": 0}


def row_pass(t, b, inv, dt=F64):
    """lse over the columns: out[i] = log sum_k exp(t[i,k] inv + b[k])."""
    t = np.asarray(t, dt)
    x = t * dt(inv) + (dt(0) if b is None else np.asarray(b, dt)[None, :])
    lse, m, e, s = _lse(x, 1)
    return lse, {"x": x, "z": t * dt(inv), "m": m, "e": e, "s": s, "lse": lse, "axis": 1}


def inv_temp(tt):
    """1 / tau of the fp32 temperature the C ABI receives, unrounded: the library's 1.0f / tau is its fp32 value (``dt(inv)`` in an
    fp32 evaluation), and that rounding is one of the counted operations of bound_pass."""
    return 1.0 / f32(tt)


def sk_center(t, tt, iters, dt=F64, trace=None):
    """The log-domain recurrence.  -> centre [K] = -tau b_iters.  ``trace`` (a list) receives the parts of every pass, in order."""
    inv, a, b = inv_temp(tt), None, None
    for n in range(1, iters + 1):
        lse, parts = col_pass(t, a, inv, dt)
        b = -lse
        if trace is not None:
            trace.append(parts)
        if n < iters:
            lse, parts = row_pass(t, b, inv, dt)
            a = -lse
            if trace is not None:
                trace.append(parts)
    return dt(f32(tt)) * -b


def targets(t, center, tt, dt=F64):
    """softmax_k((t - c) / tau), what the cross-entropy kernels form from a centre."""
    z = (np.asarray(t, dt) - np.asarray(center, dt)[None, :]) / dt(f32(tt))
    e = np.exp(z - z.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


# ------------------------------------------------------------------------------------------ fp32 error bounds
def col_adds(R):
    """Adds on the longest path to a column's sum.  Scalar kernel: the chunk's min(R, 32) rows in a row; vector kernel: 8 per slice and
    2 to join the four slices (fewer).  Then the chunks in order: ceil(R / 32) adds, each term first multiplied by exp(m_c - M) (1)."""
    return min(R, CHUNK) + -(-R // CHUNK) + 1


def row_adds(K):
    """A 256-thread strided sum (block_adds); the float4 kernel adds its four components one by one: 4 ceil(K / 1024) <= ceil(K / 256) + 3."""
    return block_adds(K) + 3


def bound_pass(parts, carried=0.0):
    """Elementwise bound of one pass' lse, given ``carried`` = the sup-norm bound of the vector a (or b) it was fed.
      argument of every exp: x - M, x = fma(t, inv, a): inv rounded (1), the fma (1), the subtraction (1):  (3 + 2) u (|z| + |a| + |M|)
      the positive sum: the weighted mean of the argument errors, then (adds + 2) u relative; a column pass also rescales every chunk by
        exp(m_c - M): argument (1 + 2) u (|m_c| + |M|) <= 6 u max|x| relative
      M + log S and the output scale (-1, or tau): (2 + 2) u (|M| + |log S|)
      expf / logf: the project's CE_LOSS_RTOL, relative to S (absolute in log S) and to log S
    lse is 1-Lipschitz in the sup norm of a: ``carried`` enters as it is."""
    x, m, e, s, lse, axis = parts["x"], parts["m"], parts["e"], parts["s"], parts["lse"], parts["axis"]
    n = x.shape[axis]
    off = np.abs(x - parts["z"])                                       # |a| (or |b|) broadcast
    da = (3 + 2) * U * (np.abs(parts["z"]) + off + np.abs(m))
    adds = col_adds(n) if axis == 0 else row_adds(n)
    rel = ((e * da).sum(axis, keepdims=True) / s + (adds + 2) * U).squeeze(axis)
    if axis == 0:
        rel = rel + 6 * U * np.abs(x).max(axis)
    logs = np.log(s).squeeze(axis)
    return carried + rel + (2 + 2) * U * (np.abs(m.squeeze(axis)) + logs) + CE_LOSS_RTOL * (1.0 + logs) + TINY


def bound_center(t, tt, iters):
    """-> (centre in float64, its elementwise bound): the bound of pass n is the sup of the bound of pass n - 1 plus the local one,
    through all 2 iters - 1 passes, times tau (the product with tau is the output scale of the last pass, counted there)."""
    trace = []
    c = sk_center(t, tt, iters, trace=trace)
    carried = 0.0
    for parts in trace:
        b = bound_pass(parts, carried)
        carried = float(b.max())
    return c, f32(tt) * b


def bound_targets(q, center_bound, tt):
    """Targets softmax((t - c) / tau) under a centre that is off by at most D = max center_bound: every argument moves by <= D / tau
    and so does the row's log-sum-exp, so log p moves by <= 2 D / tau:  |dp| <= p expm1(2 D / tau)."""
    return np.asarray(q, F64) * np.expm1(2.0 * float(np.max(center_bound)) / f32(tt)) + TINY


# ------------------------------------------------------------------------------------------ seeded inputs shared by the two test files
def sk_inputs(regime, R, K, seed):
    """fp32 teacher logits [R,K] and the teacher temperature.  normal / onehot: the teacher rows of dino_inputs (onehot: one column of
    every row stands 500 temperatures above the rest).  wide: uniform in +-20 at tau = 0.04, z in +-500: almost every term underflows."""
    if regime == "wide":
        return np.random.default_rng(seed).uniform(-20, 20, (R, K)).astype(np.float32), 0.04
    return dino_inputs(regime, R, R, K, seed)[1], 0.04
