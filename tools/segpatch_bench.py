#!/usr/bin/env python3
"""Time of the patch sampler (csrc/segpatch.hip, ops.seg_patch_sample) against the host path it replaces and a plain-torch restatement on
the same GPU, by the method of tools/segblend_bench.py: whole calls between HIP events, ROUNDS windows of back-to-back calls after a
warm-up, each at least MIN_S seconds; median with min and max.

Shape: B = 16 patches of S = 224 from 512 x 512 planes (a pool of 64), random affine jobs drawn by dinox.patches.draw_patch_jobs at its
defaults (scale 0.7-1.4, +-15 degrees, mirrors, gamma on 30 %, gain on 15 %).
  native   ops.seg_patch_sample, job tables uploaded inside the call as in training.  Bytes: what the algorithm needs, computed from the
           shapes -- each output pixel reads 4 fp32 taps and 1 label byte at most (17 B; neighbouring pixels share taps, so this is an
           upper figure for reads) and writes 3 fp32 and 1 byte (13 B) -- over the call time, as a fraction of 6.3 TB/s.
  torch    F.affine_grid + F.grid_sample on the same planes, once bilinear (image, padding zeros) and once nearest (mask as fp32), then
           gamma, gain, normalisation and the 255 outside: what a user would write without the kernel.  It needs planes of one size.
  host     the previous path: finetune_segmentation.paired_transform on 512 x 512 items through a DataLoader of batch 16, with
           min(16, cpus) persistent workers: whole passes after one warm pass, in items / s (measured before the GPU is opened).
The timing runs in a child process under its own time limit; the parent never opens the GPU.  One JSON line at the end.

    python tools/segpatch_bench.py            [ROUNDS=5 MIN_S=0.2 TIMEOUT=420]
"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUNDS = int(os.environ.get("ROUNDS", 5))
MIN_S = float(os.environ.get("MIN_S", 0.2))
TIMEOUT = int(os.environ.get("TIMEOUT", 420))
B, S, H, W, N_PLANES, CLASSES = 16, 224, 512, 512, 64, 4
HBM_ACHIEVABLE = 6.3e12


def timed(torch, fn, min_s):
    """Time per call (ms): HIP events around one window of back-to-back calls lasting at least min_s seconds."""
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    reps = max(2, int(min_s * 1e3 / max(a.elapsed_time(b), 1e-3)) + 1)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def host_items_per_s(torch, fs, workers):
    """paired_transform as the DataLoader of finetune_segmentation.py runs it: items / s of whole passes (16 batches) over persistent workers."""
    class Items(torch.utils.data.Dataset):
        def __init__(self):
            g = torch.Generator().manual_seed(0)
            self.img = torch.rand((8, H, W), generator=g)
            self.msk = torch.randint(0, CLASSES, (8, H, W), generator=g).to(torch.uint8)
            self.gen = torch.Generator().manual_seed(1)

        def __len__(self):
            return 16 * B

        def __getitem__(self, i):
            return fs.paired_transform(self.img[i % 8].expand(3, -1, -1), self.msk[i % 8], S, self.gen, True)

    loader = torch.utils.data.DataLoader(Items(), batch_size=B, num_workers=workers, drop_last=True, persistent_workers=workers > 0)
    for _ in loader:                                        # one whole pass first: the workers are started and warm, and they stay
        pass
    rates = []
    for _ in range(ROUNDS):                                 # a round is a WHOLE pass, timed from before the first request to the last batch:
        t0, n = time.perf_counter(), 0                      # nothing prefetched outside the window, no worker start-up inside it
        for x, _ in loader:
            n += x.shape[0]
        rates.append(n / (time.perf_counter() - t0))
    return rates


def worker():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "dino-x_amd"), os.path.join(ROOT, "dino-x_amd", "scripts")]
    import numpy as np
    import torch
    import torch.nn.functional as F
    import finetune_segmentation as fs
    from dinox import _lib, ops, patches as PT
    workers = min(16, os.cpu_count() or 1)
    host = host_items_per_s(torch, fs, workers)
    print(f"host     {statistics.median(host):9.1f} items/s on {workers} workers (min {min(host):.1f}, max {max(host):.1f})", flush=True)
    assert torch.cuda.is_available(), "segpatch_bench needs a GPU"
    rng = np.random.default_rng(0)
    imgs = [rng.random((H, W), dtype=np.float32) for _ in range(N_PLANES)]
    msks = [rng.integers(0, CLASSES, size=(H, W)).astype(np.uint8) for _ in range(N_PLANES)]
    pool = PT.PatchPool(imgs, msks, device="cuda")
    d = PT.draw_patch_jobs(pool, B, torch.Generator().manual_seed(0), S=S, t=S)
    mean, std = fs.fl.MEAN, fs.fl.STD

    def native():
        return ops.seg_patch_sample(pool.img, pool.msk, d["jobs"], d["par"], S, mean, std)

    planes_i, planes_m = pool.img.view(N_PLANES, 1, H, W), pool.msk.view(N_PLANES, 1, H, W)
    idx = torch.from_numpy(d["sample"]).cuda()
    par = torch.from_numpy(d["par"]).cuda()
    # theta of F.affine_grid (align_corners=False): output base coordinates (2 ox + 1) / S - 1 = 2 dx / S; input 2 sx / W - 1
    A = par[:, :6].view(B, 2, 3).clone()
    theta = torch.stack([torch.stack([A[:, 0, 0] * S / W, A[:, 0, 1] * S / W, 2 * A[:, 0, 2] / W - 1], 1),
                         torch.stack([A[:, 1, 0] * S / H, A[:, 1, 1] * S / H, 2 * A[:, 1, 2] / H - 1], 1)], 1)
    gam, gain = par[:, 6].view(B, 1, 1, 1), par[:, 7].view(B, 1, 1, 1)
    mt, st = torch.tensor(mean, device="cuda").view(1, 3, 1, 1), torch.tensor(std, device="cuda").view(1, 3, 1, 1)

    def plain():
        grid = F.affine_grid(theta, (B, 1, S, S), align_corners=False)
        v = F.grid_sample(planes_i[idx], grid, mode="bilinear", padding_mode="zeros", align_corners=False)
        lab = F.grid_sample(planes_m[idx].float() + 1, grid, mode="nearest", padding_mode="zeros", align_corners=False)
        m = torch.where(lab > 0, lab - 1, torch.full_like(lab, 255.0)).to(torch.uint8)[:, 0]
        return (gain * v.clamp_min(0).pow(gam) - mt) / st, m

    (xn, mn), (xp, mp) = native(), plain()
    row = {"what": f"B={B} S={S} planes {H}x{W} pool={N_PLANES}", "labels_agree": round(float((mn == mp).float().mean()), 6),
           "max_abs_image_difference": float((xn - xp).abs().max()),
           "host": {"items_per_s": round(statistics.median(host), 1), "min": round(min(host), 1), "max": round(max(host), 1), "workers": workers}}
    for name, fn in (("native", native), ("torch", plain)):
        ts = [timed(torch, fn, MIN_S) for _ in range(ROUNDS)]
        row[name] = {"ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4),
                     "items_per_s": round(B / statistics.median(ts) * 1e3, 1)}
        print(f"{name:8s} {row[name]['ms']:9.4f} ms per call (min {row[name]['min_ms']:.4f}, max {row[name]['max_ms']:.4f}), "
              f"{row[name]['items_per_s']:.1f} items/s", flush=True)
    rd, wr = B * S * S * 17, B * S * S * 13
    row["native"].update(bytes_read_upper=rd, bytes_written=wr, hbm_fraction=round((rd + wr) / (row["native"]["ms"] * 1e-3) / HBM_ACHIEVABLE, 5))
    print(json.dumps({"tool": "segpatch_bench", "library": os.path.basename(_lib.LIB_PATH), "rounds": ROUNDS, "min_s": MIN_S, "results": [row]}))


def main():
    if "--worker" in sys.argv:
        return worker()
    try:
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker"], timeout=TIMEOUT).returncode
    except subprocess.TimeoutExpired:
        print(f"segpatch_bench: the timing step did not finish in {TIMEOUT} s", file=sys.stderr)
        rc = 124
    sys.exit(rc)


if __name__ == "__main__":
    main()
