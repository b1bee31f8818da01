"""Worker of test_sinkhorn_gpu.py::test_rccl_call_surface_world1: ops.sk_center and one TrainEngine step with centering="sinkhorn", first
without a process group, then with every collective going through the backend (DINOX_DP_FORCE_COLLECTIVES=1, WORLD_SIZE=1).  Writes both
results to argv[1]; the test compares them."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "dino-x_amd")]

from dinox import ops  # noqa: E402
from dinox.dp import exchanging, init_process_group  # noqa: E402
from dinox.engine import StepHyperParams, TrainEngine  # noqa: E402
import zoo.arch as arch  # noqa: E402

dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
g = torch.Generator().manual_seed(5)
t = (2 * torch.randn(10, 260, generator=g)).to(dev)
t_odd = (2 * torch.randn(7, 257, generator=g)).to(dev)               # the scalar kernels
kw = dict(img_size=56, patch=14, dim=64, depth=2, heads=2, num_registers=4, scale_aware=True)
B = 4
x = torch.randn(2 * B, 3, 56, 56, generator=g).to(dev)
sp = (torch.rand(B, 3, generator=g) + 0.5).repeat(2, 1).to(dev)


def centres(group):
    return [ops.sk_center(t, 0.04, 1, group=group), ops.sk_center(t, 0.04, 3, group=group), ops.sk_center(t_odd, 0.04, 3, group=group)]


def engine_step():
    torch.manual_seed(100)
    student = arch.DinoStudentTeacher(arch.PatchViT(**kw), 256)
    torch.nn.init.xavier_uniform_(student.backbone.scale_embed.mlp[2].weight)
    teacher = arch.DinoStudentTeacher(arch.PatchViT(**kw), 256)
    teacher.load_state_dict(student.state_dict())
    hp = StepHyperParams(lr=1e-3, warmup_steps=1, max_steps=10, ema=0.99, koleo_weight=0.1, centering="sinkhorn")
    eng = TrainEngine(student.to(dev), teacher.to(dev), 256, hp, bucket_bytes=64 << 10)
    student.train()
    eng.step(x, sp)
    return eng, eng.scalars()


assert not exchanging(None)                                           # no process group yet: the single-rank forms
plain = centres(None)
_, scalars_plain = engine_step()

init_process_group()
group = torch.distributed.group.WORLD
assert exchanging(group)
grouped = centres(group)
eng, scalars = engine_step()
assert eng.bucketer.exchange
torch.save({"backend": torch.distributed.get_backend(), "exchanging": exchanging(group),
            "c1": (plain[0].cpu(), grouped[0].cpu()), "c3": (plain[1].cpu(), grouped[1].cpu()), "c3_odd": (plain[2].cpu(), grouped[2].cpu()),
            "scalars": scalars, "scalars_plain": scalars_plain}, sys.argv[1])
torch.distributed.barrier()
torch.distributed.destroy_process_group()
