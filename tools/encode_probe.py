#!/usr/bin/env python3
"""Latency of zoo.encode.encode (one image), throughput of encode_batch with host and with device preprocessing, and of
encode_volume, on ViT-S/16 224 (the inference surface of the drop-in).  Every timed window ends in a device synchronise;
repeated windows are reported as median [min .. max]."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dino-x_amd")]
import numpy as np, torch
import zoo.arch as arch
from zoo.encode import encode, encode_batch, preprocess
m = arch.PatchViT(img_size=224, patch=16, dim=384, depth=12, heads=6, num_registers=4, scale_aware=True).to("cuda").eval()
r = np.random.default_rng(0)
img = (r.standard_normal((512, 512)) * 300).astype(np.float32)
for _ in range(3): encode(m, img, pixel_spacing=(0.7, 0.7), slice_thickness=2.0)
torch.cuda.synchronize(); t0 = time.perf_counter()
for _ in range(20): f = encode(m, img, pixel_spacing=(0.7, 0.7), slice_thickness=2.0)
torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / 20
t1 = time.perf_counter()
for _ in range(20): x = preprocess(img, 224, "hu_float", 40.0, 400.0)
tp = (time.perf_counter() - t1) / 20
print(f"encode(1 x 512x512): {dt*1e3:.2f} ms per call (host preprocess alone {tp*1e3:.2f} ms)")
imgs = [img] * 64; sps = [(0.7, 0.7, 2.0)] * 64
for _ in range(2): encode_batch(m, imgs, sps)
torch.cuda.synchronize(); t0 = time.perf_counter()
for _ in range(5): encode_batch(m, imgs, sps)
torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / 5
x = torch.randn(64, 3, 224, 224, device="cuda"); sp = torch.rand(64, 3, device="cuda") + 0.5
with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
    for _ in range(3): m(x, spacing=sp)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(10): m(x, spacing=sp)
    torch.cuda.synchronize(); df = (time.perf_counter() - t0) / 10
    m32 = None
with torch.no_grad():
    for _ in range(3): m(x, spacing=sp)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(10): m(x, spacing=sp)
    torch.cuda.synchronize(); d32 = (time.perf_counter() - t0) / 10
print(f"encode_batch(64): {dt*1e3:.1f} ms = {64/dt:.0f} img/s;  forward alone on 64 device-resident images: bf16 {df*1e3:.2f} ms, fp32 {d32*1e3:.2f} ms")

# ---- device preprocessing (csrc/encode_prep.hip): the same call with preprocess="device", host and device windows alternating
import contextlib
from dinox import preprocess as P
from zoo.encode import encode_volume
QUICK = "--quick" in sys.argv                      # the profiler's run: fewer windows


def window(fn, reps):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(reps): fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def spread(ts):
    return f"{np.median(ts)*1e3:.2f} ms [{min(ts)*1e3:.2f} .. {max(ts)*1e3:.2f}]"


imgs = [(r.standard_normal((512, 512)) * 300).astype(np.float32) for _ in range(64)]       # 64 DIFFERENT arrays: 64 MiB to pack and copy
amp = lambda: torch.autocast("cuda", dtype=torch.bfloat16)
for name, ctx in (("fp32", contextlib.nullcontext), ("bf16 autocast", amp)):
    with ctx():
        for mode in ("host", "device"):
            encode_batch(m, imgs, sps, preprocess=mode)
        th, td = [], []
        for _ in range(2 if QUICK else 5):
            th.append(window(lambda: encode_batch(m, imgs, sps, preprocess="host"), 2))
            td.append(window(lambda: encode_batch(m, imgs, sps, preprocess="device"), 2))
    print(f"encode_batch(64 x 512x512 f32) {name}: host path {spread(th)} = {64/np.median(th):.0f} img/s;  device path {spread(td)} = "
          f"{64/np.median(td):.0f} img/s")
# where the device path's time goes: packing into page-locked memory (host), copy + kernel (device events)
jobs, layout, max_side = P.plane_jobs(imgs)
buf = torch.empty(layout.sizes["float32"], dtype=torch.float32, pin_memory=True)
tpk = []
for _ in range(5):
    t0 = time.perf_counter()
    host = buf.numpy()
    for im, (_, off, shape) in zip(imgs, layout.placements): np.copyto(host[off:off + im.size].reshape(shape), im)
    tpk.append(time.perf_counter() - t0)
e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
out = torch.empty(64, 3, 224, 224, device="cuda")
tc, tk = [], []
for _ in range(6):
    e[0].record(); src = buf.to("cuda", non_blocking=True); e[1].record()
    P.device_preprocess(src, jobs, 64, 224, "hu_float", 40.0, 400.0, out=out); e[2].record()
    torch.cuda.synchronize(); tc.append(e[0].elapsed_time(e[1]) * 1e-3); tk.append(e[1].elapsed_time(e[2]) * 1e-3)
moved = 64 * 512 * 512 * 4 + out.numel() * 4
print(f"  device path split: pack {spread(tpk)}, H2D copy of {buf.numel()*4/2**20:.0f} MiB {spread(tc[1:])}, table upload + kernel {spread(tk[1:])} "
      f"(kernel moves {moved/2**20:.0f} MiB: source planes once + fp32 output)")

# ---- encode_volume: a (300, 512, 512) int16 series against encode_batch over host-built 2.5D stacks of the same volume
vol = (r.standard_normal((300, 512, 512)) * 300).astype(np.int16)
sp3 = (0.7, 0.7, 2.0)


def host_stacks():
    Z = vol.shape[0]
    outs = []
    for at in range(0, Z, 64):
        st = [np.stack([vol[max(z - 1, 0)], vol[z], vol[min(z + 1, Z - 1)]], 0) for z in range(at, min(at + 64, Z))]
        outs.append(encode_batch(m, st, [sp3] * len(st)))
    return torch.cat(outs, 0)


for name, ctx in (("fp32", contextlib.nullcontext), ("bf16 autocast", amp)):
    with ctx():
        a = encode_volume(m, vol, sp3); b = host_stacks()
        rel = ((a - b).abs().max() / b.abs().max()).item()
        tv, ts = [], []
        for _ in range(1 if QUICK else 3):
            tv.append(window(lambda: encode_volume(m, vol, sp3), 1))
            ts.append(window(host_stacks, 1))
    print(f"encode_volume(300 x 512x512 i16) {name}: {spread(tv)} = {300/np.median(tv):.0f} slices/s;  encode_batch over host-built stacks "
          f"{spread(ts)} = {300/np.median(ts):.0f} slices/s  (max abs difference {rel:.1e} of the max abs feature)")
