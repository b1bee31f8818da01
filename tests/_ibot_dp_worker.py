"""Worker of the data-parallel iBOT tests: two TrainEngine steps (fp32, DINO + Gram + the masked-patch term) on this rank's shard of a
fixed global batch with a fixed global mask, of which the ranks hold different numbers of rows (rank 1 of two: none in its first view
half).  Run with RANK / WORLD_SIZE / MASTER_* set (WORLD_SIZE=1: the whole batch).  DINOX_TEST_CENTERING picks the centring.
DINOX_TEST_IDLE=1: on the second step only the samples of rank 0 are masked, so rank 1 of two holds NO masked row there and still has to
take part in every collective of the step (the zero sums of the patch centre, Sinkhorn's all-gathers, mask_token's gradient bucket)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "dino-x_amd")]

from dinox.dp import init_process_group, shard_range  # noqa: E402
from dinox.engine import StepHyperParams, TrainEngine  # noqa: E402
from dinox.ibot import make_mask  # noqa: E402
import zoo.arch as arch  # noqa: E402

rank, world, local = init_process_group()
dev = torch.device("cuda", local % torch.cuda.device_count())
torch.cuda.set_device(dev)
kw = dict(img_size=56, patch=14, dim=64, depth=2, heads=2, num_registers=4, scale_aware=True, mask_token=True)
torch.manual_seed(100)
student = arch.DinoStudentTeacher(arch.PatchViT(**kw), 256)
torch.nn.init.xavier_uniform_(student.backbone.scale_embed.mlp[2].weight)
teacher = arch.DinoStudentTeacher(arch.PatchViT(**kw), 256)
teacher.load_state_dict(student.state_dict())
hp = StepHyperParams(lr=1e-3, warmup_steps=1, max_steps=10, ema=0.99, ibot_weight=1.0, centering=os.environ.get("DINOX_TEST_CENTERING") or "ema")
eng = TrainEngine(student.to(dev), teacher.to(dev), 256, hp, bucket_bytes=64 << 10)
student.train()
g = torch.Generator().manual_seed(7)
B, P, R = 8, 16, 4
v1, v2 = torch.randn(B, 3, 56, 56, generator=g), torch.randn(B, 3, 56, 56, generator=g)
sp = torch.rand(B, 3, generator=g) * 2 + 0.4
# global views 0..B-1 = view 1 of every sample, B..2B-1 = view 2.  Masked: samples 0-2 and 5 in view 1 (none of rank 1's samples 4-7 but
# one), samples 1 and 6 in view 2: with two ranks 18 rows on rank 0 and 9 on rank 1
r = np.random.default_rng(3)
cells = {0: 5, 1: 3, 2: 7, 5: 1, B + 1: 3, B + 6: 8}
flat = np.concatenate([v * P + np.sort(r.choice(P, n, replace=False)) for v, n in cells.items()])
lo, hi = shard_range(B, rank, world)
Bl = hi - lo
gv = np.concatenate([np.arange(lo, hi), B + np.arange(lo, hi)])                     # global view of every local view
local_of = {int(v): j for j, v in enumerate(gv)}


def local_mask(flat_idx):
    mine = np.array([local_of[int(f // P)] * P + int(f % P) for f in flat_idx if int(f // P) in local_of], np.int64)
    return make_mask(mine, 2 * Bl, P, R).to(dev)


mask = local_mask(flat)
masks = [mask, mask]
if os.environ.get("DINOX_TEST_IDLE"):
    masks[1] = local_mask([f for f in flat if int(f // P) % B < B // 2])           # samples 0 .. 3 only: all of them on rank 0 of two
batch = torch.cat([v1[lo:hi], v2[lo:hi]], 0).to(dev)
sp2 = torch.cat([sp[lo:hi], sp[lo:hi]], 0).to(dev)
for m in masks:
    eng.step(batch, sp2, patch_mask=m)
sc = eng.scalars()
torch.save({"flat_p": eng.flat_p.cpu(), "center": eng.center.cpu(), "ibot_center": eng.ibot_center.cpu(), "loss": sc["loss"], "ibot": sc["ibot"],
            "grad_norm": sc["grad_norm"], "rows": mask.count, "rows_last": masks[1].count, "fired_in_backward": eng.bucketer.fired_in_backward,
            "buckets": len(eng.bucketer.buckets)}, sys.argv[1])
if torch.distributed.is_initialized():
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()
