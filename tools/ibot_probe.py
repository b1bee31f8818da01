#!/usr/bin/env python3
"""Launches of dinox_ibot_ce at the headline shape (M = 15 360 masked rows, K = 8192 prototypes) and, as the yardstick, of
dinox_sk_row_lse on one matrix of that shape -- a workload for the profiler, in runs of their own:
    rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/ibot_probe.py             kernel times
    rocprofv3 --pmc FETCH_SIZE --output-format csv -d OUT -- python tools/ibot_probe.py --calls 5   bytes read (then WRITE_SIZE)
`--summarise TRACE.csv` prints the median duration per kernel family of a kernel trace and the rate over the algorithmic bytes
(3 M K 4 for the cross-entropy with ds: s and t in, ds out; M K 4 for the row pass)."""
import argparse
import collections
import csv
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=15360)
ap.add_argument("--cols", type=int, default=8192)
ap.add_argument("--calls", type=int, default=30)
ap.add_argument("--summarise", metavar="TRACE.csv")
args = ap.parse_args()
M, K = args.rows, args.cols

if args.summarise:
    dur = collections.defaultdict(list)
    for r in csv.DictReader(open(args.summarise)):
        name = r["Kernel_Name"].split("(")[0].replace("void ", "").replace("dinox::", "")
        dur[name].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    need = {"ibot_ce_reg_kernel": 3 * M * K * 4, "sk_row_lse_kernel": M * K * 4}
    out = {}
    for name, ts in sorted(dur.items()):
        fam = name.split("<")[0]
        if fam.startswith(("ibot_", "sk_row")):
            ts = sorted(ts[3:])                        # (the first launches load the code object)
            med = ts[len(ts) // 2]
            out[name] = {"launches": len(ts), "median_us": round(med, 2), "min_us": round(ts[0], 2), "max_us": round(ts[-1], 2)}
            if fam in need:
                out[name]["algorithmic_TB_per_s"] = round(need[fam] / med / 1e6, 3)
    print(json.dumps(out, indent=1))
    sys.exit(0)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dino-x_amd")]
import torch  # noqa: E402
from dinox import ops  # noqa: E402

g = torch.Generator(device="cuda").manual_seed(0)
s = 2 * torch.randn(M, K, device="cuda", generator=g)
t = 2 * torch.randn(M, K, device="cuda", generator=g)
c = torch.zeros(K, device="cuda")
w = torch.full((M,), 1.0 / 60, device="cuda")
ds = torch.empty_like(s)
for _ in range(args.calls):
    ops.ibot_ce(s, t, c, w, 0.1, 0.04, scale=1.0 / 512, ds_out=ds)
    ops.sk_row_lse(t, None, 25.0, 1.0)
torch.cuda.synchronize()
print(f"ibot_probe: {args.calls} calls of ibot_ce and sk_row_lse at {M} x {K}")
