"""Every compiled path of csrc/lora.hip on the GPU: the case table of tests/_lora_paths_cases.py (its coverage of the launch decisions is
shown on the CPU by tests/test_lora_paths_cpu.py) against the float64 oracle and the bounds of tests/_lora_oracle.py.

The C entries are called directly so that the test owns every address.  Inputs live inside buffers of NaN (before, after, and in the
skipped leading element of a misaligned operand): a value read from past a row or column end and USED makes the output NaN.  Outputs live
inside buffers of the fp32 canary word: every word around them must survive, none inside may be left.  dinox_lora_grad gets exactly
dinox_lora_grad_ws_bytes of workspace between canaries.  Each case runs on four value families (randn, cancel, range, zeroB), twice (the
second launch must repeat the first bit for bit), and a misaligned case must equal its aligned twin bit for bit: the scalar and the vector
loads of stage_tile / dot_tile feed the same values to the same instructions in the same order, up's r4 loop and its scalar-j loop run the
same chain in ascending j, and VEC = 1 and VEC = 4 apply `s * acc (+ res)` to each element alone.  No pair's order differs, so none is
held to the bound only.
"""
import numpy as np
import pytest
import torch

import _lora_oracle as LO
import _lora_paths_cases as LP
from oracle.gemm_bounds import CANARY_F32

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
G = 64                      # guard elements on either side: 128 bytes of bf16, 256 of fp32, so a view's alignment is its offset's
CANARY = int(CANARY_F32)
RATIOS: dict = {}           # entry -> largest error / bound (DESIGN.md records them)
_RESULTS: dict = {}         # (case name, family) -> {output: int32 bits on the host}


def _dt(c):
    return torch.bfloat16 if c["dtype"] == "bf16" else torch.float32


def put_in(a, dt, off, need):
    """``a`` inside a NaN buffer, ``off`` elements past a 256-byte boundary -> (buffer, address).  ``need``: the alignment in bytes the
    operand's vector form asks for; the address is held to it (off = 0) or off it (off = 1)."""
    a = np.ascontiguousarray(a, np.float32).reshape(-1)
    buf = torch.full((G + off + a.size + G,), float("nan"), dtype=dt, device=DEV)
    view = buf[G + off:G + off + a.size]
    view.copy_(torch.from_numpy(a).to(dt))
    assert np.array_equal(view.float().cpu().numpy(), a)                                   # (bf16 operands hold bf16-exact values)
    ptr = view.data_ptr()
    assert buf.data_ptr() % 256 == 0 and ptr % 16 == (off * buf.element_size()) % 16 and (ptr % need == 0) == (off == 0), (ptr, off, need)
    return buf, ptr


class Out:
    """n fp32 outputs inside canary words, ``off`` words past a 256-byte boundary."""

    def __init__(self, n, off, init=None):
        self.n, self.lo = n, G + off
        self.buf = torch.full((G + off + n + G,), CANARY, dtype=torch.int32, device=DEV)
        if init is not None:                                                               # in place: the output starts as res / W
            self.buf[self.lo:self.lo + n].view(torch.float32).copy_(torch.from_numpy(np.ascontiguousarray(init, np.float32).reshape(-1)))
        self.ptr = self.buf.data_ptr() + 4 * self.lo
        assert self.buf.data_ptr() % 256 == 0 and self.ptr % 16 == (4 * off) % 16 and (self.ptr % 16 == 0) == (off == 0)

    def bits(self, what):
        body = self.buf[self.lo:self.lo + self.n]
        assert bool((self.buf[:self.lo] == CANARY).all()) and bool((self.buf[self.lo + self.n:] == CANARY).all()), f"{what}: written outside the buffer"
        assert not bool((body == CANARY).any()), f"{what}: an output element was left unwritten"
        return body.clone()


def launch(c, o):
    """One call of the case's entry on fresh buffers -> {output name: int32 bits on the device}."""
    from dinox import _lib
    from dinox.ops import _code, _stream
    L, off, e = _lib.lib, set(c["off"]), c["entry"]
    M, K, N, r, dt = c["M"], c["K"], c["N"], c["r"], _dt(c)
    act_need = 8 if c["dtype"] == "bf16" else 16
    f = torch.float32
    keep = []                                                                              # the buffers stay alive until the synchronize

    def inp(name, a, d=f, need=16):
        buf, ptr = put_in(a, d, int(name in off), need)
        keep.append(buf)
        return ptr

    if e == "down":
        S = o["S"] if c["layout"] == 0 else o["S"].T
        u = Out(M * r, int("u" in off))
        outs = {"u": u}
        rc = L.dinox_lora_down(inp("x", o["x"], dt, act_need), inp("S", S), u.ptr, M, K, r, c["layout"], _code(dt), _stream())
    elif e == "up":
        S = o["S"] if c["layout"] == 0 else o["S"].T
        t = Out(M * N, int("t" in off), init=o["res"] if c["res"] == "inplace" else None)
        outs = {"t": t}
        if c["res"] == "inplace":
            assert ("res" in off) == ("t" in off)
        res = None if c["res"] == "none" else t.ptr if c["res"] == "inplace" else inp("res", o["res"])
        rc = L.dinox_lora_up(inp("u", o["u"]), inp("S", S), res, t.ptr, c["s"], M, N, r, c["layout"], _stream())
    elif e == "grad":
        nws = L.dinox_lora_grad_ws_bytes(M, K, N, r)
        assert nws == 4 * -(-M // LO.CHUNK) * (r * K + N * r)
        dA, dB, ws = Out(r * K, 0), Out(N * r, 0), Out(nws // 4, 0)                        # exactly the bytes the library asks for
        outs = {"dA": dA, "dB": dB, "ws": ws}
        rc = L.dinox_lora_grad(inp("xl", o["xl"], dt, act_need), inp("dy", o["dy"], dt, act_need), inp("A", o["A"]), inp("B", o["B"]), c["s"],
                               dA.ptr, dB.ptr, ws.ptr, M, K, N, r, _code(dt), _stream())
    else:
        out = Out(N * K, int("out" in off), init=o["W"] if c["res"] == "inplace" else None)
        outs = {"out": out}
        if c["res"] == "inplace":
            assert ("W" in off) == ("out" in off)
        w = out.ptr if c["res"] == "inplace" else inp("W", o["W"])
        rc = L.dinox_lora_merge(w, inp("A", o["A"]), inp("B", o["B"]), out.ptr, c["s"], c["sign"], N, K, r, _stream())
    _lib.check(rc, f"dinox_lora_{e}")
    torch.cuda.synchronize()
    return {k: v.bits(f"{c['name']} {k}") for k, v in outs.items()}


def run(c, family):
    """The case on one family: two launches (equal bits), every output inside its bound -> ({output: bits on the host}, worst ratio)."""
    key = (c["name"], family)
    if key in _RESULTS:
        return _RESULTS[key]
    o = LP.make(c, family)
    first, second = launch(c, o), launch(c, o)
    worst = 0.0
    for k, (ref, bound) in LO.reference(c, o).items():
        assert torch.equal(first[k], second[k]), f"{key} {k}: the second launch differs"
        got = first[k].view(torch.float32).double().cpu().numpy().reshape(ref.shape)
        assert not np.isnan(got).any(), f"{key} {k}: NaN (a padding value was used)"
        assert np.isfinite(got).all(), f"{key} {k}: non-finite output"
        err = np.abs(got - ref)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(err == 0.0, 0.0, err / bound)
        ratio = float(q.max())
        worst = max(worst, ratio)
        assert (err <= bound).all(), f"{key} {k}: error / bound = {ratio:.3g} at {np.unravel_index(q.argmax(), q.shape)}"
    if c["entry"] == "grad":
        assert torch.equal(first["ws"], second["ws"])
    if family == "zeroB":                                                                  # exactly 0.0, not small
        bits = {k: v.view(torch.float32) for k, v in first.items()}
        if c["entry"] == "down":
            assert torch.count_nonzero(bits["u"]) == 0
        elif c["entry"] == "grad":
            assert torch.count_nonzero(bits["dA"]) == 0 and torch.count_nonzero(bits["dB"]) > 0
        else:
            k, base = ("t", "res") if c["entry"] == "up" else ("out", "W")
            addend = bits[k] - torch.from_numpy(o[base].reshape(-1)).to(DEV) if c["res"] != "none" else bits[k]
            assert torch.count_nonzero(addend) == 0
    _RESULTS[key] = ({k: v.cpu() for k, v in first.items() if k != "ws"}, worst)
    return _RESULTS[key]


@pytest.mark.parametrize("name", [c["name"] for c in LP.CASES])
def test_case(name):
    c = LP.BY_NAME[name]
    per = {}
    for family in LP.FAMILIES:
        bits, per[family] = run(c, family)
        if c["twin"]:
            twin, _ = run(LP.BY_NAME[c["twin"]], family)
            for k in bits:
                assert torch.equal(bits[k], twin[k]), f"{name} {family} {k}: differs from its aligned form {c['twin']}"
    worst = max(per.values())
    RATIOS[c["entry"]] = max(RATIOS.get(c["entry"], 0.0), worst)
    tags = ",".join(sorted(t.split(":", 1)[1] for t in LP.case_paths(c)))
    print(f"LORA-PATHS {c['entry']} {name} {tags}: ratio={worst:.4f} (" + " ".join(f"{f}={v:.4f}" for f, v in per.items()) + ")")
    assert worst <= 1.0


def test_zz_report_largest_ratios():
    """Not a check of its own: prints the largest error / bound ratio per entry (each was asserted <= 1 above)."""
    for k in sorted(RATIOS):
        print(f"LORA-PATHS largest ratio  {k:6s} {RATIOS[k]:.4f}")
    assert all(v <= 1.0 for v in RATIOS.values())
