"""Host side of the device-preprocessing path of zoo.encode (dinox/preprocess.py, encode_volume): job tables, the filter rule the
kernel is written from, the golden fixture against the host code, argument errors.  No kernel is launched here."""
import json

import numpy as np
import pytest
import torch

from conftest import load_golden

MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32).reshape(3, 1, 1)
STD = np.array([0.229, 0.224, 0.225], dtype=np.float32).reshape(3, 1, 1)


@pytest.fixture(scope="module")
def gold():
    g = load_golden("encode_preprocess.npz")
    return g, json.loads(str(g["cases"]))


def clamp_triples(Z, zs):
    return [(max(z - 1, 0), z, min(z + 1, Z - 1)) for z in zs]


def coverage(jobs, H, W):
    """{destination: plane} of a volume job table; asserts <= 3 destinations per job and that none repeats."""
    seen = {}
    for off, h, w, rs, ps, nd, *d in jobs.tolist():
        assert (h, w, rs, ps) == (H, W, W, 1) and off % (H * W) == 0 and 1 <= nd <= 3
        assert all(v == -1 for v in d[nd:])
        for dst in d[:nd]:
            assert dst not in seen, f"destination {dst} written twice"
            seen[dst] = off // (H * W)
    return seen


# ---------------------------------------------------------------- 1. plane_jobs
def test_plane_jobs_mixed_list(gold):
    from dinox.preprocess import plane_jobs
    g, _ = gold
    images = [g["in_a"], g["in_b"], g["in_c"], g["in_d"]]
    jobs, layout, max_side = plane_jobs(images)
    assert jobs.dtype == np.int64 and jobs.shape == (1 + 3 + 3 + 1, 9)
    assert max_side == 131
    assert layout.job_dtype == ["float32"] + ["uint16"] * 3 + ["float32"] * 3 + ["int16"]
    assert layout.sizes == {"float32": 131 * 97 + 33 * 47 * 3, "uint16": 3 * 20 * 37, "int16": 28 * 28}
    assert layout.placements == [("float32", 0, (131, 97)), ("uint16", 0, (3, 20, 37)), ("float32", 131 * 97, (33, 47, 3)),
                                 ("int16", 0, (28, 28))]
    rows = jobs.tolist()
    assert rows[0] == [0, 131, 97, 97, 1, 3, 0, 1, 2]                                           # replicated plane: one job, three destinations
    for c in range(3):
        assert rows[1 + c] == [c * 20 * 37, 20, 37, 37, 1, 1, 3 + c, -1, -1]                  # (3, H, W): planar
        assert rows[4 + c] == [131 * 97 + c, 33, 47, 3 * 47, 3, 1, 6 + c, -1, -1]             # (H, W, 3): pixel stride 3
    assert rows[7] == [0, 28, 28, 28, 1, 3, 9, 10, 11]
    dests = sorted(d for r in rows for d in r[6:6 + r[5]])
    assert dests == list(range(12))                                                            # every (image, channel) exactly once
    assert layout.jobs_of(jobs, "uint16").tolist() == rows[1:4]


@pytest.mark.parametrize("shape", [(4,), (2, 5, 5), (5, 5, 4), (1, 2, 3, 4)])
def test_plane_jobs_bad_shape(shape):
    from dinox.preprocess import plane_jobs
    from zoo.encode import _channels
    arr = np.zeros(shape, dtype=np.float32)
    with pytest.raises(ValueError) as host:
        _channels(arr)
    with pytest.raises(ValueError) as dev:
        plane_jobs([np.zeros((4, 4), np.float32), arr])
    assert str(dev.value) == str(host.value)


# ---------------------------------------------------------------- 2. volume_jobs
@pytest.mark.parametrize("Z,zs", [(1, [0]), (2, [0, 1]), (5, [0, 1, 2, 3, 4]), (5, [0, 2, 4]), (5, [3, 1, 3, 0, 3, 3])])
def test_volume_jobs_neighbours(Z, zs):
    from dinox.preprocess import volume_jobs
    H, W = 6, 7
    seen = coverage(volume_jobs(Z, H, W, zs, "neighbours"), H, W)
    want = {3 * k + c: p for k, tri in enumerate(clamp_triples(Z, zs)) for c, p in enumerate(tri)}
    assert seen == want


def test_volume_jobs_split_and_order():
    from dinox.preprocess import volume_jobs
    jobs = volume_jobs(5, 4, 4, [3, 1, 3, 0, 3, 3], "neighbours")
    planes = [r[0] // 16 for r in jobs.tolist()]
    assert planes == sorted(planes)
    assert planes.count(3) == 2 and planes.count(2) == 2 and planes.count(4) == 2          # four copies of slice 3: each of its planes is split
    assert sum(r[5] for r in jobs.tolist()) == 18
    full = volume_jobs(5, 4, 4, range(5))
    assert len(full) == 5 and all(r[5] == 3 for r in full.tolist())                         # one resize per plane, not three


def test_volume_jobs_replicate():
    from dinox.preprocess import volume_jobs
    seen = coverage(volume_jobs(5, 6, 7, [0, 1, 2, 3, 4], "replicate"), 6, 7)
    assert seen == {3 * z + c: z for z in range(5) for c in range(3)}
    assert len(volume_jobs(5, 6, 7, [0, 1, 2, 3, 4], "replicate")) == 5


def test_volume_jobs_chunk_drops_outside_destinations():
    from dinox.preprocess import volume_jobs
    seen = coverage(volume_jobs(5, 6, 7, [2, 3], "neighbours"), 6, 7)
    assert sorted(set(seen.values())) == [1, 2, 3, 4]
    assert seen == {0: 1, 1: 2, 2: 3, 3: 2, 4: 3, 5: 4}                                     # nothing for slices 1 and 4, which also show planes 2 and 3


def test_volume_jobs_errors_and_check_jobs():
    from dinox.preprocess import check_jobs, volume_jobs
    with pytest.raises(ValueError, match="context"):
        volume_jobs(5, 4, 4, [0], "mirror")
    with pytest.raises(ValueError, match="outside"):
        volume_jobs(5, 4, 4, [5])
    jobs = volume_jobs(5, 4, 6, range(5))
    assert check_jobs(jobs, 5 * 4 * 6, 5) == 6
    with pytest.raises(ValueError, match="past the source"):
        check_jobs(jobs, 5 * 4 * 6 - 1, 5)
    with pytest.raises(ValueError, match="destination"):
        check_jobs(jobs, 5 * 4 * 6, 4)


# ---------------------------------------------------------------- 3. the filter rule
from oracle.resample_bounds import pil_bilinear_weights as axis_weights  # noqa: E402  (PIL's rule; shared with the bounds of oracle/resample_bounds.py)


def resize_rule(plane, S):
    """Separable, horizontal pass first, fp32 intermediate, fp32 accumulation."""
    H, W = plane.shape
    mid = np.zeros((H, S), dtype=np.float32)
    for i, (x0, w) in enumerate(axis_weights(W, S)):
        acc = np.zeros(H, dtype=np.float32)
        for k, wk in enumerate(w.astype(np.float32)):
            acc += wk * plane[:, x0 + k]
        mid[:, i] = acc
    out = np.zeros((S, S), dtype=np.float32)
    for i, (y0, w) in enumerate(axis_weights(H, S)):
        acc = np.zeros(S, dtype=np.float32)
        for k, wk in enumerate(w.astype(np.float32)):
            acc += wk * mid[y0 + k, :]
        out[i] = acc
    return out


def windowed_planes(raw, fmt, level, width):
    """Steps 1-3 of the kernel on the host, in fp32: three (H, W) planes in [0, 1]."""
    a = raw.astype(np.float32)
    if fmt == "hu16_png":
        a = (a - np.float32(32768.0)) * np.float32(0.1)
    if fmt != "windowed_float":
        lo, hi = level - width / 2, level + width / 2
        a = (np.clip(a, np.float32(lo), np.float32(hi)) - np.float32(lo)) / np.float32(hi - lo)
    if a.ndim == 2:
        return [a, a, a]
    return [a[:, :, c] for c in range(3)] if a.shape[2] == 3 else [a[c] for c in range(3)]


def test_equal_size_weights_are_exact():
    for x0, w in axis_weights(28, 28):
        assert w[0] == 1.0 and (w[1:] == 0.0).all()


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e"])
def test_filter_rule_reproduces_golden(gold, name):
    g, cases = gold
    case = next(c for c in cases if c["name"] == name)
    planes = windowed_planes(g[f"in_{name}"], case["format"], case["level"], case["width"])
    got = np.stack([resize_rule(np.ascontiguousarray(p), case["S"]) for p in planes], 0).astype(np.float64)
    want = g[f"out_{name}"].astype(np.float64) * STD.astype(np.float64) + MEAN.astype(np.float64)       # back on the [0, 1] image
    err = np.abs(got - want).max()
    print(f"case {name}: filter rule vs reference, max abs on the [0, 1] image {err:.3e}")
    assert err <= 2.4e-7                                                                                  # 2 ulp at 1.0


# ---------------------------------------------------------------- 4. the host path against the fixture
@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e"])
def test_host_preprocess_equals_golden_bitwise(gold, name):
    from zoo.encode import preprocess
    g, cases = gold
    case = next(c for c in cases if c["name"] == name)
    got = preprocess(g[f"in_{name}"], case["S"], case["format"], case["level"], case["width"])
    assert got.dtype == torch.float32 and torch.equal(got, torch.from_numpy(g[f"out_{name}"]))


# ---------------------------------------------------------------- 5. arguments
class CpuStub:
    """A model on the CPU that records its input (the HIP engine itself computes only on a GPU)."""
    img_size, scale_aware = 16, False

    def __init__(self):
        self.seen = None

    def parameters(self):
        return iter([torch.zeros(1)])

    def __call__(self, x, spacing=None):
        self.seen = x
        return torch.zeros(x.shape[0], 3, 8)


def test_encode_volume_argument_errors():
    from zoo.encode import encode_volume
    m, vol = CpuStub(), np.zeros((4, 8, 8), dtype=np.int16)
    with pytest.raises(ValueError, match="volume shape"):
        encode_volume(m, vol[0], (1.0, 1.0, 1.0))
    with pytest.raises(ValueError, match="volume shape"):
        encode_volume(m, vol[None], (1.0, 1.0, 1.0))
    with pytest.raises(ValueError, match="Unknown input_format"):
        encode_volume(m, vol, (1.0, 1.0, 1.0), input_format="dicom")
    with pytest.raises(ValueError, match="Unknown context"):
        encode_volume(m, vol, (1.0, 1.0, 1.0), context="mirror")
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="z_stride"):
            encode_volume(m, vol, (1.0, 1.0, 1.0), z_stride=bad)


def test_auto_on_a_cpu_model_takes_the_host_path(monkeypatch, gold):
    import dinox.preprocess as P
    from zoo.encode import encode, encode_batch, preprocess
    g, _ = gold

    def boom(*a, **k):
        raise AssertionError("the kernel launch was reached for a model on the CPU")

    monkeypatch.setattr(P, "launch", boom)
    monkeypatch.setattr(P, "pack_and_preprocess", boom)
    m = CpuStub()
    out = encode_batch(m, [g["in_a"], g["in_e"]], [(1.0, 1.0, 1.0)] * 2, preprocess="auto")
    assert out.shape == (2, 1, 8)
    want = torch.stack([preprocess(g[k], 16, "hu_float", 40.0, 400.0) for k in ("in_a", "in_e")], 0)
    assert torch.equal(m.seen, want)
    encode(m, g["in_a"], preprocess="auto")
    assert torch.equal(m.seen, want[:1])
    with pytest.raises(ValueError, match="Unknown preprocess"):
        encode(m, g["in_a"], preprocess="gpu")


def test_device_on_a_cpu_model_is_an_error(monkeypatch, gold):
    import dinox.preprocess as P
    from zoo.encode import encode
    g, _ = gold
    monkeypatch.setattr(P, "launch", lambda *a: pytest.fail("launched"))
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        encode(CpuStub(), g["in_a"], preprocess="device")
