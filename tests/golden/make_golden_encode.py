#!/usr/bin/env python3
"""Generate encode_preprocess.npz FROM THE REAL REFERENCE (run where the reference checkout exists; it does not travel to the GPU box):

    DINOX_REFERENCE=<reference checkout> python tests/golden/make_golden_encode.py

It imports the reference's own ``zoo.encode`` and calls its ``encode`` on the CPU with a stub model that records the tensor it is
handed (the stub exposes ``img_size``, ``scale_aware = False``, ``parameters()`` and ``__call__``), i.e. the reference's NumPy + PIL
preprocessing end to end.  Per case the file holds the raw input (``in_<case>``) and the recorded ``(3, S, S)`` fp32 tensor
(``out_<case>``); ``cases`` is the JSON list of {name, format, S, level, width}.  Inputs are seeded ``default_rng`` draws:

  a  hu_float        f32 (131, 97), N(40, 300)   -> 40   non-integer downscale on both axes; 2.5 tiles of 16: ragged edge tiles; replicated plane
  b  hu16_png        u16 (3, 20, 37)             -> 28   upscale in y, downscale in x; values include 0 and 65535
  c  windowed_float  f32 (33, 47, 3)             -> 16   interleaved channels; exactly one tile
  d  hu_float        i16 (28, 28), -600 / 1500   -> 28   equal size; values exactly at lo and hi and beyond both
  e  hu_float        f32 (17, 16)                -> 32   pure upscale
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


class Recorder:
    """Stands in for the PatchViT: keeps what ``encode`` hands to the forward."""
    scale_aware = False

    def __init__(self, img_size: int) -> None:
        self.img_size, self.seen = img_size, None

    def parameters(self):
        return iter([torch.zeros(1)])

    def __call__(self, x, spacing=None):
        self.seen = x.detach().clone()
        return torch.zeros(x.shape[0], 2, 4)


def cases():
    r = np.random.default_rng(20260)
    a = (40.0 + 300.0 * r.standard_normal((131, 97))).astype(np.float32)
    b = r.integers(30000, 36000, size=(3, 20, 37)).astype(np.uint16)           # around HU 0: inside and outside the default window
    b[0, 0, 0], b[1, 3, 5], b[2, 19, 36] = 0, 65535, 0
    b[0, 7, 7], b[2, 0, 1] = 65535, 32768
    c = r.random((33, 47, 3), dtype=np.float32)
    d = r.integers(-2000, 800, size=(28, 28)).astype(np.int16)
    d[0, :4] = (-1350, 150, -1351, 151)                                         # lo, hi, one past each
    d[27, 24:] = (-32768, 32767, -1350, 150)
    e = (40.0 + 300.0 * r.standard_normal((17, 16))).astype(np.float32)
    return [("a", "hu_float", a, 40, 40.0, 400.0), ("b", "hu16_png", b, 28, 40.0, 400.0), ("c", "windowed_float", c, 16, 40.0, 400.0),
            ("d", "hu_float", d, 28, -600.0, 1500.0), ("e", "hu_float", e, 32, 40.0, 400.0)]


def main() -> None:
    ref = os.environ.get("DINOX_REFERENCE") or (sys.argv[1] if len(sys.argv) > 1 else None)
    if not ref or not os.path.isdir(os.path.join(ref, "zoo")):
        raise SystemExit("set DINOX_REFERENCE (or pass the path) to the reference checkout")
    sys.dont_write_bytecode = True
    sys.path.insert(0, ref)
    import PIL
    from zoo.encode import encode                      # (the reference)
    assert os.path.abspath(sys.modules["zoo.encode"].__file__).startswith(os.path.abspath(ref))

    arrays, meta = {}, []
    for name, fmt, raw, S, level, width in cases():
        model = Recorder(S)
        encode(model, raw, pixel_spacing=(0.7, 0.7), slice_thickness=2.0, input_format=fmt, hu_level=level, hu_width=width)
        got = model.seen
        assert got.shape == (1, 3, S, S) and got.dtype == torch.float32
        arrays[f"in_{name}"], arrays[f"out_{name}"] = raw, got[0].numpy()
        meta.append(dict(name=name, format=fmt, S=S, level=level, width=width))
        print(f"case {name}: {fmt} {raw.dtype} {raw.shape} -> {S}: out in [{got.min():.4f}, {got.max():.4f}]")
    out = os.path.join(HERE, "encode_preprocess.npz")
    np.savez_compressed(out, cases=np.array(json.dumps(meta)), pil_version=np.array(PIL.__version__), **arrays)
    print(f"wrote {out} ({os.path.getsize(out)} bytes)")


if __name__ == "__main__":
    main()
