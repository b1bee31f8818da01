"""The device-preprocessing path of zoo.encode on an MI355X: csrc/encode_prep.hip against the fixture recorded from the reference's
own encode (tests/golden/make_golden_encode.py), encode_volume against encode_batch over host-built stacks, the decline path and
the command-line script."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
MEAN = torch.tensor([0.485, 0.456, 0.406]).view(3, 1, 1)
STD = torch.tensor([0.229, 0.224, 0.225]).view(3, 1, 1)
# The fp32 restatement of the filter rule sits within 1.2e-7 of PIL on the [0, 1] image (test_encode_device_cpu.py); divided by the
# smallest std (0.224) that is 5e-7 on the normalised tensor.  The gate leaves ~20x for fp32 weight arithmetic on the device.
GATE = 1e-5
SP = (0.7, 0.7, 2.0)


class Recorder:
    """A model on the GPU that keeps the batch it is handed: shows what the preprocessing made, without a forward."""
    scale_aware = False

    def __init__(self, img_size):
        self.img_size, self.seen = img_size, None

    def parameters(self):
        return iter([torch.zeros(1, device=DEV)])

    def __call__(self, x, spacing=None):
        self.seen = x.clone()
        return torch.zeros(x.shape[0], 2, 4, device=DEV)


@pytest.fixture(scope="module")
def gold():
    g = load_golden("encode_preprocess.npz")
    return g, {c["name"]: c for c in json.loads(str(g["cases"]))}


@pytest.fixture(scope="module")
def tiny():
    import zoo.arch as arch
    torch.manual_seed(5)
    m = arch.PatchViT(img_size=28, patch=14, dim=64, depth=2, heads=2, scale_aware=True)
    with torch.no_grad():
        torch.nn.init.normal_(m.scale_embed.mlp[2].weight, std=0.2)           # zero-initialised: let the spacing reach the tokens
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def volume():
    return np.random.default_rng(11).integers(-400, 500, size=(5, 24, 30)).astype(np.int16)


def stacks(vol):
    Z = vol.shape[0]
    return [np.stack([vol[max(z - 1, 0)], vol[z], vol[min(z + 1, Z - 1)]], 0) for z in range(Z)]


def device_batch(images, S, fmt="hu_float", level=40.0, width=400.0):
    from zoo.encode import encode_batch
    m = Recorder(S)
    encode_batch(m, images, [SP] * len(images), input_format=fmt, hu_level=level, hu_width=width, preprocess="device")
    return m.seen.cpu()


def rel_gate(got, want):
    return (got - want).abs().max().item() / want.abs().max().item()


# ---------------------------------------------------------------- 1. - 3. the kernel against the golden cases
@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e"])
def test_kernel_matches_reference_case(gold, name):
    g, cases = gold
    c = cases[name]
    got = device_batch([g[f"in_{name}"]], c["S"], c["format"], c["level"], c["width"])[0]
    err = (got - torch.from_numpy(g[f"out_{name}"])).abs().max().item()
    print(f"case {name}: device vs reference, max abs on the normalised tensor {err:.3e}")
    assert err <= GATE


def test_mixed_batch_in_one_call(gold):
    """All five raw inputs in ONE encode_batch call: three source dtypes (grouped into one launch each), three layouts, five shapes.
    The format, the window and S are per-call arguments, so the call runs at case a's (hu_float, 40 / 400, S = 40): image 0 is held to the
    fixture, every image to the host code -- bitwise the reference's arithmetic (test_encode_device_cpu.py) -- at the same gate, and
    the batch equals the five single-image launches bitwise."""
    from zoo.encode import preprocess
    g, _ = gold
    images = [g[f"in_{n}"] for n in "abcde"]
    batch = device_batch(images, 40)
    want = torch.stack([preprocess(im, 40, "hu_float", 40.0, 400.0) for im in images], 0)
    err = (batch - want).abs().max().item()
    print(f"mixed batch of five at S = 40: device vs host, max abs {err:.3e}")
    assert err <= GATE
    assert (batch[0] - torch.from_numpy(g["out_a"])).abs().max().item() <= GATE
    for k, im in enumerate(images):
        assert torch.equal(device_batch([im], 40)[0], batch[k])


def test_equal_size_is_bitwise_the_host_path(gold):
    from zoo.encode import preprocess
    g, cases = gold
    c = cases["d"]
    got = device_batch([g["in_d"]], c["S"], c["format"], c["level"], c["width"])[0]
    assert torch.equal(got, preprocess(g["in_d"], c["S"], c["format"], c["level"], c["width"]))
    assert torch.equal(got, torch.from_numpy(g["out_d"]))


def test_replicated_plane_is_one_job_three_destinations(gold):
    g, cases = gold
    got = device_batch([g["in_a"]], cases["a"]["S"])[0]
    v = got * STD + MEAN                                      # back before the normalisation: the same plane three times
    ulp = float(np.spacing(np.float32(1.0)))
    assert (v[0] - v[1]).abs().max().item() <= ulp and (v[0] - v[2]).abs().max().item() <= ulp
    assert not torch.equal(got[0], got[1])                    # (and each channel got its own mean / std)


# ---------------------------------------------------------------- 4. volume
@pytest.fixture(scope="module")
def volume_reference(tiny, volume):
    """encode_batch with host preprocessing over the five explicitly stacked triples: computed once, shared, never changed."""
    from zoo.encode import encode_batch
    return encode_batch(tiny, stacks(volume), [SP] * 5).cpu()


def test_encode_volume_equals_host_built_stacks(tiny, volume, volume_reference):
    from zoo.encode import encode_volume
    got = encode_volume(tiny, volume, SP).cpu()
    assert got.shape == (5, 1, 64)
    rel = rel_gate(got, volume_reference)
    print(f"encode_volume vs encode_batch(host stacks): {rel:.3e} of the max abs feature")
    assert rel <= 1e-3
    chunked = encode_volume(tiny, volume, SP, batch_size=2).cpu()
    assert rel_gate(chunked, volume_reference) <= 1e-3
    tokens = encode_volume(tiny, volume, SP, return_all_tokens=True)
    assert tokens.shape == (5, 1 + 4 + tiny.num_registers, 64) and torch.equal(tokens[:, 0:1].cpu(), got)


def test_volume_input_is_the_same_in_any_chunking(volume):
    from dinox.preprocess import device_preprocess, volume_jobs
    src = torch.from_numpy(volume).reshape(-1).to(DEV)
    whole = device_preprocess(src, volume_jobs(5, 24, 30, range(5)), 5, 28, "hu_float", 40.0, 400.0)
    parts = [device_preprocess(src, volume_jobs(5, 24, 30, ch), len(ch), 28, "hu_float", 40.0, 400.0) for ch in ([0, 1], [2, 3], [4])]
    assert torch.equal(torch.cat(parts, 0), whole)
    from zoo.encode import preprocess
    want = torch.stack([preprocess(s, 28, "hu_float", 40.0, 400.0) for s in stacks(volume)], 0)
    assert (whole.cpu() - want).abs().max().item() <= GATE


def test_encode_volume_stride_and_replicate(tiny, volume, volume_reference):
    from zoo.encode import encode_batch, encode_volume
    got = encode_volume(tiny, volume, SP, z_stride=2).cpu()
    assert got.shape == (3, 1, 64)
    assert rel_gate(got, volume_reference[0::2]) <= 1e-3
    rep = encode_volume(tiny, volume, SP, context="replicate").cpu()
    want = encode_batch(tiny, [volume[z] for z in range(5)], [SP] * 5).cpu()
    assert rel_gate(rep, want) <= 1e-3


# ---------------------------------------------------------------- 5. decline, not fault
def test_oversized_source_declines_before_any_launch(tiny):
    from dinox.preprocess import lds_bytes
    from zoo.encode import encode_batch
    img = np.random.default_rng(3).standard_normal((3000, 8)).astype(np.float32) * 300
    m = Recorder(8)
    assert lds_bytes(8, 3000) > 150 * 1024
    with pytest.raises(RuntimeError, match="LDS"):
        encode_batch(m, [img], [SP], preprocess="device")
    assert m.seen is None
    encode_batch(m, [img], [SP], preprocess="auto")
    encode_auto = m.seen.cpu()
    encode_batch(m, [img], [SP])
    assert torch.equal(encode_auto, m.seen.cpu())


# ---------------------------------------------------------------- 6. strided and float64 input
def test_strided_and_float64_input(gold):
    g, _ = gold
    base = np.random.default_rng(8).standard_normal((70, 120)) * 300 + 40          # float64
    view = base.astype(np.float32)[::2, ::3]
    assert not view.flags["C_CONTIGUOUS"]
    want = device_batch([np.ascontiguousarray(view)], 24)
    assert torch.equal(device_batch([view], 24), want)
    f64 = base[::2, ::3]
    assert f64.dtype == np.float64
    assert torch.equal(device_batch([f64], 24), want)
    inter = np.random.default_rng(9).integers(0, 65535, size=(40, 33, 6)).astype(np.uint16)[:, :, ::2]       # (H, W, 3), strided pixels
    assert torch.equal(device_batch([inter], 24, "hu16_png"), device_batch([np.ascontiguousarray(inter)], 24, "hu16_png"))


# ---------------------------------------------------------------- 7. the script
def test_encode_volume_script(tiny, volume, tmp_path):
    from zoo.encode import encode_volume
    cfg = dict(img_size=28, patch=14, dim=64, depth=2, heads=2, mlp_ratio=4.0, num_registers=tiny.num_registers, scale_aware=True)
    torch.save({"model": {k: v.cpu() for k, v in tiny.state_dict().items()}, "config": {"model": cfg}}, tmp_path / "ckpt.pth")
    np.save(tmp_path / "vol.npy", volume)
    out = tmp_path / "emb.npy"
    cmd = [sys.executable, os.path.join(ROOT, "dino-x_amd", "scripts", "encode_volume.py"), "--checkpoint", str(tmp_path / "ckpt.pth"),
           "--volume", str(tmp_path / "vol.npy"), "--spacing", *(str(v) for v in SP), "--batch-size", "2", "--out", str(out)]
    run = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert run.returncode == 0, run.stdout
    assert "slices=5 " in run.stdout and "slices_per_s=" in run.stdout
    emb = np.load(out)
    assert emb.shape == (5, 64) and emb.dtype == np.float32
    want = encode_volume(tiny, volume, SP, batch_size=2)[:, 0].cpu().numpy()
    assert np.array_equal(emb, want)
