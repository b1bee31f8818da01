"""Guarded, poisoned allocations for the workspace-contract tests (a helper, not a conftest: nothing happens at import).

`with guarded(poison) as g:` replaces torch.empty for the duration of the block.  Every call then
  * allocates the requested bytes plus GUARD = 4096 bytes on each side (4096 is a multiple of 256, so the live view keeps the base
    alignment; `data_ptr() % 256 == 0` is asserted because the seg, GEMM and LayerNorm dispatch reads pointer alignment and the guard
    must not move a case onto another kernel),
  * fills both guards with the canary word and every byte of the live region with `poison`,
  * returns the live view with the requested shape, dtype and device, and records it.
On exit (and on demand) `g.check()` asserts that every canary byte of every recorded allocation is intact; a failure names the
allocation (index, byte size, the caller's file:line from inspect) and the first damaged offset relative to the live region.

Poisons: 0xFF is NaN in fp32 / bf16 / fp64 and -1 in the integer types; 0x7F is ~3.39e38 in fp32, large and finite in bf16, positive
in the integer types.  fmaxf drops a NaN, so a max-reduction over unwritten scratch shows only under 0x7F.

Not intercepted: torch.zeros, torch.full, empty_like, new_empty, Tensor.new_*; DESIGN.md ("Workspace contract") lists the wrappers
that use them.  Cached workspaces (ops._TN_WS, ops._BLOCK_TN_WS) were allocated earlier and bypass the guard: drop_caches() empties
them, and guarded() calls it on entry unless told not to.
"""
import contextlib
import inspect
import os

import torch

GUARD = 4096
ALIGN = 256
CANARY = 0x5AC3A596                      # the canary word; its bytes 96 A5 C3 5A repeat from the first byte of either guard
POISON_NAN, POISON_BIG = 0xFF, 0x7F
POISONS = (POISON_NAN, POISON_BIG)
_HERE = os.path.abspath(__file__)
_CANARY_BYTES: dict = {}


def drop_caches():
    """Forget every workspace dinox.ops keeps between calls, so that the next call allocates again (through the patched torch.empty)."""
    from dinox import ops
    ops._TN_WS.clear()
    ops._BLOCK_TN_WS.clear()


def canary_bytes(device):
    """GUARD bytes of the canary word on `device` (built once per device with torch.full, never through torch.empty)."""
    key = str(device)
    if key not in _CANARY_BYTES:
        _CANARY_BYTES[key] = torch.full((GUARD // 4,), CANARY, dtype=torch.int32, device=device).view(torch.uint8)
    return _CANARY_BYTES[key]


def _call_site():
    f = inspect.currentframe()
    try:
        while f is not None and os.path.abspath(f.f_code.co_filename) == _HERE:
            f = f.f_back
        return "?" if f is None else f"{os.path.basename(f.f_code.co_filename)}:{f.f_lineno} in {f.f_code.co_name}"
    finally:
        del f


class Allocation:
    __slots__ = ("index", "nbytes", "site", "raw", "lo", "live")

    def __init__(self, index, nbytes, site, raw, lo, live):
        self.index, self.nbytes, self.site, self.raw, self.lo, self.live = index, nbytes, site, raw, lo, live

    def guards(self):
        a, b = self.lo, self.lo + GUARD + self.nbytes
        return self.raw[a:a + GUARD], self.raw[b:b + GUARD]

    def damage(self):
        """None, or the first damaged canary byte as an offset from the start of the live region (negative: in front of it)."""
        want = canary_bytes(self.raw.device)
        for guard, base in zip(self.guards(), (-GUARD, self.nbytes)):
            if not torch.equal(guard, want):
                return base + int((guard != want).nonzero()[0])
        return None


class Guard:
    def __init__(self, poison, real_empty):
        assert poison in range(256)
        self.poison, self.allocations, self._real = poison, [], real_empty

    def empty(self, *size, dtype=None, device=None, **kw):
        """The replacement of torch.empty."""
        if kw.get("out") is not None or kw.get("pin_memory") or kw.get("layout", torch.strided) is not torch.strided:
            return self._real(*size, dtype=dtype, device=device, **kw)
        if len(size) == 1 and not isinstance(size[0], int):
            size = tuple(size[0])
        shape = tuple(int(s) for s in size)
        dtype = dtype or torch.get_default_dtype()
        nbytes = self._real((), dtype=dtype, device="meta").element_size()
        for s in shape:
            assert s >= 0, shape
            nbytes *= s
        raw = self._real(nbytes + 2 * GUARD + ALIGN, dtype=torch.uint8, device=device)
        lo = (-raw.data_ptr()) % ALIGN                                # 0 on the device (the caching allocator hands out 512-byte blocks)
        live = raw[lo + GUARD:lo + GUARD + nbytes]
        live.fill_(self.poison)
        live = live.view(dtype).view(shape)
        assert live.data_ptr() % ALIGN == 0 and live.is_contiguous() and live.shape == shape and live.dtype == dtype
        a = Allocation(len(self.allocations), nbytes, _call_site(), raw, lo, live)
        for guard in a.guards():
            guard.copy_(canary_bytes(raw.device))
        if kw.get("requires_grad"):
            live.requires_grad_(True)
        self.allocations.append(a)
        return live

    def damaged(self):
        """[(allocation, first damaged offset)] over every recorded allocation."""
        return [(a, d) for a in self.allocations for d in [a.damage()] if d is not None]

    def check(self):
        bad = self.damaged()
        assert not bad, "canary damaged: " + "; ".join(
            f"allocation #{a.index} ({a.nbytes} bytes, from {a.site}) first at live{d:+d}" for a, d in bad)

    def __len__(self):
        return len(self.allocations)


@contextlib.contextmanager
def guarded(poison, drop=True, check=True):
    """torch.empty -> guarded, poisoned allocations for the duration of the block; restored on exit whatever happens.  The caches of
    dinox.ops are dropped first (drop=False: keep them, for the test that shows why).  check=False leaves the canary check to the
    caller (g.check() / g.damaged())."""
    if drop:
        drop_caches()
    real = torch.empty
    g = Guard(poison, real)
    torch.empty = g.empty
    try:
        yield g
    finally:
        torch.empty = real
    if any(a.raw.is_cuda for a in g.allocations):
        torch.cuda.synchronize()
    if check:
        g.check()


def as_bytes(t):
    """The tensor's storage as a flat uint8 CPU tensor: equality of these is bit equality (NaN == NaN)."""
    return t.detach().contiguous().reshape(-1).view(torch.uint8).cpu()


def poisoned_elements(t, poison):
    """Boolean CPU tensor, shape of t: True where every byte of the element equals the poison byte."""
    t = t.detach().contiguous()
    b = t.reshape(-1).view(torch.uint8).cpu().reshape(t.numel(), t.element_size())
    return (b == poison).all(1).reshape(t.shape)
