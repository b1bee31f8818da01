"""The case table of tests/test_lora_paths_gpu.py / test_lora_paths_cpu.py and a host-only restatement of the launch decisions of
csrc/lora.hip: which flags the entry points compute (vec, svec, vecK, vecN, avec, VEC, r4), how many 128-column tiles, 32-wide rank
blocks, 128-row chunks and 4-row groups a call walks and how each of them ends.  ``paths(...)`` returns the tags one call takes,
``ALL_PATHS`` is the full set written out from the source, ``CASES`` the smallest shapes that reach all of it.

Several tags are JOINT on purpose.  "a second tile" and "a ragged end" were both reached before this table existed (K = 384 and K = 36),
only never by the same call: the code that runs for ``c0 > 0`` with ``col >= C`` is reached by neither.  So the tile tag names the number of
tiles and the end of the last one together, the rank tag the number of blocks and whether the last is full, the row tag the number of
chunks and the last chunk's fill.

How a tile ends (w = width of the last tile): ``full`` w = 128; ``ragged:8`` a whole number of dot_tile's 8-column g steps; ``ragged:4`` a
whole 4-column group more (the h = 1 half of the last g step is past the end: ``col < C`` is false for 32 lanes of every wave);
``ragged:in4`` the end lies inside a 4-column group (only without the vector forms: C % 4 != 0, the ``col + i < C`` guards decide).

``off`` names the operands that sit one element past a 16-byte aligned address (2 bytes in bf16, 4 in fp32: either way off the 8- or
16-byte alignment the vector form of that operand needs).  Operand names: down x S u; up u S res t; grad xl dy A B; merge W A B out.
"""
import numpy as np

TILE = 128            # csrc/lora.hip LT_COLS
CHUNK = 128           # LT_ROWS = LORA_GRAD_CHUNK
UP_ROWS = 4           # rows per thread of lora_up_kernel
UP_THREADS = 256

FAMILIES = ("randn", "cancel", "range", "zeroB")


# ------------------------------------------------------------------------------------------ the predicate
def _tiles(C):
    nt = -(-C // TILE)
    w = C - (nt - 1) * TILE
    end = "full" if w == TILE else "ragged:8" if w % 8 == 0 else "ragged:4" if w % 4 == 0 else "ragged:in4"
    return f"tiles{'1' if nt == 1 else 'N'}:{end}", w


def _rows(M):
    n = -(-M // CHUNK)
    last = M - (n - 1) * CHUNK
    return f"rows:chunks{'1' if n == 1 else 'N'}:{'full' if last == CHUNK else 'single' if last == 1 else 'ragged'}"


def _njb(r):
    return ("njb1:" + ("full" if r == 32 else "partial")) if r <= 32 else ("njb2:" + ("full" if r == 64 else "partial"))


def _flag(name, width_ok, aligned):
    return f"{name}:on" if width_ok and aligned else f"{name}:off:{'align' if width_ok else 'width'}"


def _pass2(w):
    """Pass 2 of lora_grad_partial_kernel on the last tile: wave w works iff c0 + 32 w < C (all four / some idle); a working wave's 32
    columns are all inside (whole) or cut by ``col < C`` (partial)."""
    return f"pass2:{'all' if w > 96 else 'idle'}:{'whole' if w % 32 == 0 else 'partial'}"


def _up(rows, cols, r, layout, off_u, off_S, off_res, off_t, has_res, names):
    """lora_up (shared by dinox_lora_up and dinox_lora_merge): VEC, r4, the rank's remainder, the 4-row groups and the grid."""
    nu, nS, nres, nt = names
    if cols % 4:
        vec = "VEC1:width"
    elif off_t:
        vec = f"VEC1:align:{nt}"
    elif has_res and off_res:
        vec = f"VEC1:align:{nres}"
    elif layout == 1 and off_S:
        vec = f"VEC1:align:{nS}"
    else:
        vec = "VEC4"
    if layout == 1:
        r4 = "r4:off:layout"
    elif r % 4:
        r4 = "r4:off:rank"
    elif off_u:
        r4 = f"r4:off:align:{nu}"
    elif off_S:
        r4 = f"r4:off:align:{nS}"
    elif vec != "VEC4":
        r4 = "r4:off:VEC1"                       # the flag is set, the VEC = 1 instantiation compiles the loop out
    else:
        r4 = "r4:on"
    items = -(-rows // UP_ROWS) * (cols // 4 if vec == "VEC4" else cols)
    grid = f"grid{'1' if items <= UP_THREADS else 'N'}:{'full' if items % UP_THREADS == 0 else 'tail'}"
    return {vec, r4, "r:1" if r == 1 else "r:rem" if r % 4 else "r:mult4",
            "rows:single" if rows == 1 else "rows:full4" if rows % UP_ROWS == 0 else "rows:clamped", grid}


def paths(entry, M, K, N, r, dtype, layout, off=(), res="none", sign=1):
    """The tags of one call.  down: x [M,K], S [r,K] (layout 0) or [K,r] (1).  up: u [M,r], S [N,r] (0) or [r,N] (1), ``res`` one of
    none / given / inplace.  grad: xl [M,K], dy [M,N], A [r,K], B [N,r].  merge: W [N,K], A [r,K], B [N,r], res given / inplace."""
    off = set(off)
    if entry == "down":
        t = {dtype, f"layout{layout}", _flag("vec", K % 4 == 0, "x" not in off),
             "svec:off:layout" if layout == 1 else _flag("svec", K % 4 == 0, "S" not in off), _njb(r), "K:" + _tiles(K)[0], _rows(M)}
    elif entry == "up":
        t = _up(M, N, r, layout, "u" in off, "S" in off, "res" in off, "t" in off, res != "none", ("u", "S", "res", "t"))
        t |= {f"layout{layout}", f"res:{res}"}
    elif entry == "merge":
        t = _up(N, K, r, 1, "B" in off, "A" in off, "W" in off, "out" in off, True, ("B", "A", "W", "out"))
        t = {x for x in t if not x.startswith("grid")} | {"inplace" if res == "inplace" else "outofplace", "sign+" if sign > 0 else "sign-"}
    elif entry == "grad":
        (tk, wk), (tn, wn) = _tiles(K), _tiles(N)
        t = {dtype, _flag("vecK", K % 4 == 0, "xl" not in off), _flag("vecN", N % 4 == 0, "dy" not in off),
             _flag("avec", K % 4 == 0, "A" not in off), "bvec:off:layout", _njb(r), "K:" + tk, "N:" + tn, "K:" + _pass2(wk), "N:" + _pass2(wn),
             _rows(M)}
    else:
        raise ValueError(entry)
    return {f"{entry}:{x}" for x in t}


# ------------------------------------------------------------------------------------------ every tag, by hand from csrc/lora.hip
_TILE_ENDS = ["tiles1:full", "tiles1:ragged:8", "tiles1:ragged:4", "tiles1:ragged:in4", "tilesN:full", "tilesN:ragged:8", "tilesN:ragged:4",
              "tilesN:ragged:in4"]
_ROW_ENDS = ["rows:chunks1:full", "rows:chunks1:ragged", "rows:chunks1:single", "rows:chunksN:full", "rows:chunksN:ragged", "rows:chunksN:single"]
_NJB = ["njb1:full", "njb1:partial", "njb2:full", "njb2:partial"]
_PASS2 = ["pass2:all:whole", "pass2:all:partial", "pass2:idle:whole", "pass2:idle:partial"]
_UP_COMMON = ["r:1", "r:rem", "r:mult4", "rows:single", "rows:full4", "rows:clamped"]

ALL_PATHS = set(
    # dinox_lora_down: DX_LAUNCH by dtype and layout; vec / svec of the entry; chunk_dot's tile loop, dot_tile's rank blocks; one workgroup a chunk
    ["down:" + x for x in ["f32", "bf16", "layout0", "layout1", "vec:on", "vec:off:width", "vec:off:align", "svec:on", "svec:off:width",
                           "svec:off:align", "svec:off:layout"] + _NJB + ["K:" + e for e in _TILE_ENDS] + _ROW_ENDS]
    # dinox_lora_up: lora_up()'s vec and r4, the kernel's two j loops, the clamped rows, the last workgroup
    + ["up:" + x for x in ["layout0", "layout1", "VEC4", "VEC1:width", "VEC1:align:t", "VEC1:align:res", "VEC1:align:S", "r4:on", "r4:off:rank",
                           "r4:off:align:u", "r4:off:align:S", "r4:off:layout", "r4:off:VEC1", "grid1:full", "grid1:tail", "gridN:full",
                           "gridN:tail", "res:none", "res:given", "res:inplace"] + _UP_COMMON]
    # dinox_lora_grad: both chunk_dot calls (A in layout 0 with avec, B in layout 1 without a vector form), pass 2 on both axes
    + ["grad:" + x for x in ["f32", "bf16", "vecK:on", "vecK:off:width", "vecK:off:align", "vecN:on", "vecN:off:width", "vecN:off:align", "avec:on",
                             "avec:off:width", "avec:off:align", "bvec:off:layout", "bvec:on"] + _NJB + ["K:" + e for e in _TILE_ENDS]
       + ["N:" + e for e in _TILE_ENDS] + ["K:" + p for p in _PASS2] + ["N:" + p for p in _PASS2] + _ROW_ENDS]
    # dinox_lora_merge: lora_up() with B as the rows, A [r][K] in layout 1, W as res
    + ["merge:" + x for x in ["VEC4", "VEC1:width", "VEC1:align:W", "VEC1:align:out", "VEC1:align:A", "r4:off:layout", "r4:on", "inplace",
                              "outofplace", "sign+", "sign-"] + _UP_COMMON])

UNREACHABLE = {
    "merge:r4:on": "dinox_lora_merge always passes layout 1 (A is stored [r][K]); r4 needs layout 0 and the LAYOUT 1 kernels compile its loop out",
    "grad:bvec:on": "lora_grad_partial_kernel calls chunk_dot<DT, 1> for dy B with svec = false: layout 1 has no vector form in dot_tile",
}


# ------------------------------------------------------------------------------------------ the cases
def _c(name, entry, M, K=0, N=0, r=8, dtype="f32", layout=0, off=(), res="none", sign=1, s=0.375, twin=None):
    return dict(name=name, entry=entry, M=M, K=K, N=N, r=r, dtype=dtype, layout=layout, off=tuple(off), res=res, sign=sign, s=s, twin=twin)


# K, N from {8, 36, 128, 130, 132, 200, 260, 384} plus 6 (the only way to end a FIRST tile inside a 4-group: 8 and 36 are multiples of 4),
# 100 and 160 (pass 2 with all four waves at work and the last one cut, and with idle waves beside whole ones: no width of the list has a
# last tile of 97 .. 127 or of 32 / 64 / 96 columns); M from {1, 5, 128, 129, 130, 257} plus 256 (several chunks, the last one full).
# ``twin``: the aligned case a misaligned one must equal bit for bit (same values, same chain order; see test_lora_paths_gpu.py).
CASES = [
    # ---- down
    _c("d-1x8-r1", "down", 1, K=8, r=1),
    _c("d-5x36-r6-bf16-l1", "down", 5, K=36, r=6, dtype="bf16", layout=1),
    _c("d-128x128-r32", "down", 128, K=128, r=32),
    _c("d-129x130-r33-bf16", "down", 129, K=130, r=33, dtype="bf16"),
    _c("d-130x132-r40-l1", "down", 130, K=132, r=40, layout=1),
    _c("d-257x200-r63-bf16-l1", "down", 257, K=200, r=63, dtype="bf16", layout=1),
    _c("d-5x260-r64", "down", 5, K=260, r=64),
    _c("d-256x384-r8-bf16", "down", 256, K=384, r=8, dtype="bf16"),
    _c("d-5x6-r1-l1", "down", 5, K=6, r=1, layout=1),
    _c("d-5x132-r8", "down", 5, K=132, r=8),
    _c("d-5x132-r8-off-x", "down", 5, K=132, r=8, off=("x",), twin="d-5x132-r8"),
    _c("d-5x132-r8-off-S", "down", 5, K=132, r=8, off=("S",), twin="d-5x132-r8"),
    _c("d-5x132-r8-off-u", "down", 5, K=132, r=8, off=("u",), twin="d-5x132-r8"),
    _c("d-5x132-r8-bf16", "down", 5, K=132, r=8, dtype="bf16"),
    _c("d-5x132-r8-bf16-off-x", "down", 5, K=132, r=8, dtype="bf16", off=("x",), twin="d-5x132-r8-bf16"),
    # ---- up
    _c("u-1x8-r1", "up", 1, N=8, r=1),
    _c("u-5x36-r6-res", "up", 5, N=36, r=6, res="given"),
    _c("u-128x128-r32-inplace", "up", 128, N=128, r=32, res="inplace"),
    _c("u-129x130-r33-res", "up", 129, N=130, r=33, res="given"),
    _c("u-130x132-r40-l1", "up", 130, N=132, r=40, layout=1),
    _c("u-257x130-r63-l1-res", "up", 257, N=130, r=63, layout=1, res="given"),
    _c("u-5x200-r64", "up", 5, N=200, r=64),
    _c("u-5x130-r8", "up", 5, N=130, r=8),
    _c("u-128x8-r8-off-t", "up", 128, N=8, r=8, off=("t",)),
    _c("u-5x132-r8-res", "up", 5, N=132, r=8, res="given"),
    _c("u-5x132-r8-res-off-u", "up", 5, N=132, r=8, res="given", off=("u",), twin="u-5x132-r8-res"),
    _c("u-5x132-r8-res-off-S", "up", 5, N=132, r=8, res="given", off=("S",), twin="u-5x132-r8-res"),
    _c("u-5x132-r8-res-off-t", "up", 5, N=132, r=8, res="given", off=("t",), twin="u-5x132-r8-res"),
    _c("u-5x132-r8-res-off-res", "up", 5, N=132, r=8, res="given", off=("res",), twin="u-5x132-r8-res"),
    _c("u-5x132-r8-inplace-off", "up", 5, N=132, r=8, res="inplace", off=("res", "t"), twin="u-5x132-r8-res"),
    _c("u-5x132-r8-l1-res", "up", 5, N=132, r=8, layout=1, res="given"),
    _c("u-5x132-r8-l1-res-off-S", "up", 5, N=132, r=8, layout=1, res="given", off=("S",), twin="u-5x132-r8-l1-res"),
    # ---- grad
    _c("g-1x8x36-r1", "grad", 1, K=8, N=36, r=1, s=1.5),
    _c("g-5x36x8-r6-bf16", "grad", 5, K=36, N=8, r=6, dtype="bf16", s=1.5),
    _c("g-128x128x384-r32", "grad", 128, K=128, N=384, r=32, s=1.5),
    _c("g-129x130x132-r33-bf16", "grad", 129, K=130, N=132, r=33, dtype="bf16", s=1.5),
    _c("g-130x132x130-r40", "grad", 130, K=132, N=130, r=40, s=1.5),
    _c("g-257x200x260-r63-bf16", "grad", 257, K=200, N=260, r=63, dtype="bf16", s=1.5),
    _c("g-5x260x200-r64", "grad", 5, K=260, N=200, r=64, s=1.5),
    _c("g-256x384x128-r8-bf16", "grad", 256, K=384, N=128, r=8, dtype="bf16", s=1.5),
    _c("g-5x100x160-r8", "grad", 5, K=100, N=160, r=8, s=1.5),
    _c("g-130x160x100-r33-bf16", "grad", 130, K=160, N=100, r=33, dtype="bf16", s=1.5),
    _c("g-5x6x6-r6", "grad", 5, K=6, N=6, r=6, s=1.5),
    _c("g-5x132x132-r8", "grad", 5, K=132, N=132, r=8, s=1.5),
    _c("g-5x132x132-r8-off-xl", "grad", 5, K=132, N=132, r=8, s=1.5, off=("xl",), twin="g-5x132x132-r8"),
    _c("g-5x132x132-r8-off-dy", "grad", 5, K=132, N=132, r=8, s=1.5, off=("dy",), twin="g-5x132x132-r8"),
    _c("g-5x132x132-r8-off-A", "grad", 5, K=132, N=132, r=8, s=1.5, off=("A",), twin="g-5x132x132-r8"),
    _c("g-5x132x132-r8-bf16", "grad", 5, K=132, N=132, r=8, dtype="bf16", s=1.5),
    _c("g-5x132x132-r8-bf16-off-xl", "grad", 5, K=132, N=132, r=8, dtype="bf16", s=1.5, off=("xl",), twin="g-5x132x132-r8-bf16"),
    _c("g-5x132x132-r8-bf16-off-dy", "grad", 5, K=132, N=132, r=8, dtype="bf16", s=1.5, off=("dy",), twin="g-5x132x132-r8-bf16"),
    # ---- merge
    _c("m-1x8-r1", "merge", 0, N=1, K=8, r=1, res="given", s=2.0),
    _c("m-5x130-r33-neg-inplace", "merge", 0, N=5, K=130, r=33, res="inplace", sign=-1, s=2.0),
    _c("m-128x132-r64-inplace", "merge", 0, N=128, K=132, r=64, res="inplace", s=2.0),
    _c("m-130x36-r6-neg", "merge", 0, N=130, K=36, r=6, res="given", sign=-1, s=2.0),
    _c("m-5x132-r8", "merge", 0, N=5, K=132, r=8, res="given", s=2.0),
    _c("m-5x132-r8-off-W", "merge", 0, N=5, K=132, r=8, res="given", s=2.0, off=("W",), twin="m-5x132-r8"),
    _c("m-5x132-r8-off-out", "merge", 0, N=5, K=132, r=8, res="given", s=2.0, off=("out",), twin="m-5x132-r8"),
    _c("m-5x132-r8-off-A", "merge", 0, N=5, K=132, r=8, res="given", s=2.0, off=("A",), twin="m-5x132-r8"),
    _c("m-5x132-r8-inplace-off", "merge", 0, N=5, K=132, r=8, res="inplace", s=2.0, off=("W", "out"), twin="m-5x132-r8"),
]
BY_NAME = {c["name"]: c for c in CASES}


def case_paths(c):
    return paths(c["entry"], c["M"], c["K"], c["N"], c["r"], c["dtype"], c["layout"], c["off"], c["res"], c["sign"])


# ------------------------------------------------------------------------------------------ the value families
def _bf16_exact(a):
    """Round to nearest-even bf16, as float32 (NumPy only)."""
    b = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return b.astype(np.uint32).view(np.float32).reshape(np.shape(a))


def _pair_cancel(rng, X, S):
    """X [rows, n], S [cols, n], contracted over n: every term of the first half is positive, the second half repeats the first in X and
    negates it (to 2^-12) in S.  Every chain climbs to half of sum |x s| -- which stays O(n) -- and comes back to ~2^-12 of it: the
    roundings happen at the magnitudes the bound is made of, the result has none of them left, and a term taken twice, dropped, or with
    the wrong sign leaves a whole term standing.  An odd n leaves one term over: it is scaled by 2^-10."""
    n = X.shape[1]
    h = n // 2
    np.abs(X, out=X)
    np.abs(S, out=S)
    X[:, h:2 * h] = X[:, :h]
    S[:, h:2 * h] = -S[:, :h] * (1.0 + 2.0 ** -12 * rng.standard_normal(S[:, :h].shape)).astype(np.float32)
    if n % 2 and n > 1:
        S[:, -1] *= np.float32(2.0 ** -10)


def _row_scale(M, sign=1):
    e = np.round(np.linspace(-20, 20, M)) if M > 1 else np.array([20.0])
    return np.exp2(sign * e).astype(np.float32)[:, None]


def make(c, family):
    """The operands of one case as float32 arrays in their MATHEMATICAL orientation (S, A [r,K]; B [N,r]; up's S [N,r]); activations of a
    bf16 case hold bf16-exact values.  Deterministic in (case name, family)."""
    seed_name = c["twin"] or c["name"]                     # a misaligned twin computes on its aligned case's values
    rng = np.random.default_rng([sum(map(ord, seed_name)), FAMILIES.index(family), c["M"], c["K"], c["N"], c["r"]])
    g = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    M, K, N, r, e = c["M"], c["K"], c["N"], c["r"], c["entry"]
    if e == "down":
        o = dict(x=g(M, K), S=g(r, K))
        if family == "cancel":
            _pair_cancel(rng, o["x"], o["S"])
        if family == "range":
            o["x"] *= _row_scale(M)
        if family == "zeroB":
            o["S"][:] = 0.0
        acts = ("x",)
    elif e == "up":
        o = dict(u=g(M, r), S=g(N, r), res=g(M, N))
        if family == "cancel":
            _pair_cancel(rng, o["u"], o["S"])
        if family == "range":
            o["u"] *= _row_scale(M)
            o["res"] *= _row_scale(M)
        if family == "zeroB":
            o["S"][:] = 0.0
        acts = ()
    elif e == "grad":
        o = dict(xl=g(M, K), dy=g(M, N), A=g(r, K) * np.float32(0.25), B=g(N, r) * np.float32(0.25))
        if family == "cancel":
            _pair_cancel(rng, o["xl"], o["A"])
            Bt = np.ascontiguousarray(o["B"].T)
            _pair_cancel(rng, o["dy"], Bt)
            o["B"] = np.ascontiguousarray(Bt.T)
        if family == "range":                          # xl rows up, dy rows down: the products over the rows stay O(1), the operands do not
            o["xl"] *= _row_scale(M)
            o["dy"] *= _row_scale(M, -1)
        if family == "zeroB":
            o["B"][:] = 0.0
        acts = ("xl", "dy")
    else:
        o = dict(W=g(N, K), A=g(r, K) * np.float32(0.25), B=g(N, r) * np.float32(0.25))
        if family == "cancel":
            At = np.ascontiguousarray(o["A"].T)
            _pair_cancel(rng, o["B"], At)
            o["A"] = np.ascontiguousarray(At.T)
        if family == "range":
            o["W"] *= _row_scale(N)
            o["B"] *= _row_scale(N)
        if family == "zeroB":
            o["B"][:] = 0.0
        acts = ()
    if c["dtype"] == "bf16":
        for k in acts:
            o[k] = _bf16_exact(o[k])
    return o
