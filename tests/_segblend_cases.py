"""The seeded cases of tests/test_segblend_gpu.py, built here so that tests/test_segblend_cpu.py can run the oracle's fp32 emulation
over exactly the same inputs (the share of pixels the margin rule exempts is a condition of those tests, confirmed without a GPU)."""
from functools import lru_cache

import numpy as np

import _segblend_oracle as O

# (H, W, t, g, overlap): t a multiple of g with neither side a multiple of 64 (two overlaps); a non-integer factor; a factor under 2 with
# ny > 1 only just; a one-row strip; a single tile; t < g without overlap
GEOMETRIES = ((37, 53, 16, 4, 0.5), (37, 53, 16, 4, 0.75), (37, 53, 10, 4, 0.5), (9, 23, 7, 4, 0.5), (16, 41, 16, 4, 0.5), (16, 16, 16, 4, 0.5),
              (70, 70, 3, 5, 0.0))
CLASSES = (2, 3, 5, 64)
KINDS = ("randn", "randn30", "offset")
WINDOWS = ("gaussian", "constant")


def case_ids():
    return [f"{gi}-{C}" for gi in range(len(GEOMETRIES)) for C in CLASSES]


def case_spec(cid: str) -> dict:
    """Every geometry with every C; F, B, the window and the kind of logits rotate so that each value meets each geometry and each C."""
    gi, C = (int(v) for v in cid.split("-"))
    ci = CLASSES.index(C)
    H, W, t, g, overlap = GEOMETRIES[gi]
    F = (1, 4)[(gi + ci) % 2]
    flips = [int(v) for v in np.random.default_rng(100 + 4 * gi + ci).permutation(4)][:F] if F == 4 else [(0, 3, 1, 2)[(gi + ci // 2) % 4]]
    return dict(H=H, W=W, t=t, g=g, overlap=overlap, C=C, F=F, flips=flips, B=(1, 3)[(gi + ci // 2) % 2], window=WINDOWS[(gi + (ci + 1) // 2) % 2],
                kind=KINDS[(gi + 2 * ci) % 3], seed=1000 + 4 * gi + ci)


@lru_cache(maxsize=None)
def case(cid: str):
    """(spec, ys, xs, win, z fp32, oracle): computed once per case, shared, never changed."""
    from dinox.tiled import blend_window, tile_starts
    s = case_spec(cid)
    ys, xs = tile_starts(s["H"], s["t"], s["overlap"]), tile_starts(s["W"], s["t"], s["overlap"])
    win = blend_window(s["t"], s["window"])
    z = O.make_logits(s["kind"], (s["B"], s["F"], len(ys), len(xs), s["g"] ** 2, s["C"]), s["seed"])
    z.setflags(write=False)
    return s, ys, xs, win, z, O.Blend(z, ys, xs, s["flips"], win, s["H"], s["W"], s["t"])
