"""Worker of tests/test_simclr_dp_gpu.py.  argv: <mode> <output file>.

steps    Two TrainEngine steps with loss_type="simclr" (fp32 parity mode) on this rank's shard of a fixed global batch of 8 samples.
         With WORLD_SIZE > 1 (RANK / MASTER_* set, gloo: both ranks on one GPU) the negatives are global (simclr_negatives="global")
         and the ranks start from different seeds, so the broadcast matters; WORLD_SIZE = 1 is the single process at the whole batch
         on the square single-rank kernels.
surface  World of one rank, every collective through the real backend (DINOX_DP_FORCE_COLLECTIVES=1): ops.ntxent_fwd / ntxent_bwd
         and one engine step, first without a process group (the square kernels), then with it (all-gathers + rectangular kernels).
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "dino-x_amd")]

from dinox import ops  # noqa: E402
from dinox.dp import exchanging, init_process_group, shard_range  # noqa: E402
from dinox.engine import StepHyperParams, TrainEngine  # noqa: E402
import zoo.arch as arch  # noqa: E402

mode, out_path = sys.argv[1], sys.argv[2]
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
kw = dict(img_size=56, patch=14, dim=64, depth=2, heads=2, num_registers=4, scale_aware=True)
OUT = 256
g = torch.Generator().manual_seed(7)
B = 8
v1, v2 = torch.randn(B, 3, 56, 56, generator=g), torch.randn(B, 3, 56, 56, generator=g)
sp = torch.rand(B, 3, generator=g) * 2 + 0.4


def engine(seed, negatives):
    torch.manual_seed(seed)
    student = arch.DinoStudentTeacher(arch.PatchViT(**kw), OUT)
    torch.nn.init.xavier_uniform_(student.backbone.scale_embed.mlp[2].weight)
    teacher = arch.DinoStudentTeacher(arch.PatchViT(**kw), OUT)
    teacher.load_state_dict(student.state_dict())
    hp = StepHyperParams(lr=1e-3, warmup_steps=1, max_steps=10, loss_type="simclr", simclr_negatives=negatives)
    eng = TrainEngine(student.to(dev), teacher.to(dev), OUT, hp, bucket_bytes=64 << 10)
    student.train()
    return eng


def shard(lo, hi):
    return torch.cat([v1[lo:hi], v2[lo:hi]], 0).to(dev), torch.cat([sp[lo:hi], sp[lo:hi]], 0).to(dev)


if mode == "steps":
    rank, world, _ = init_process_group()
    eng = engine(100 + rank if world > 1 else 100, "global" if world > 1 else "local")
    assert (eng._ntxent_group is not None) == (world > 1) and eng.bucketer.exchange == (world > 1)
    batch, sp2 = shard(*shard_range(B, rank, world))
    for _ in range(2):
        eng.step(batch, sp2)
    sc = eng.scalars()
    torch.save({"flat_p": eng.flat_p.cpu(), "loss": sc["loss"], "simclr": sc["simclr"], "grad_norm": sc["grad_norm"]}, out_path)
elif mode == "surface":
    z = (2 * torch.randn(66, 130, generator=g)).to(dev)
    batch, sp2 = shard(0, B)

    def head(group):
        loss, saved = ops.ntxent_fwd(z, 0.1, group=group)
        return loss.cpu(), ops.ntxent_bwd(saved, 1.0).cpu(), len(saved)

    def step(negatives):
        eng = engine(100, negatives)
        eng.step(batch, sp2)
        return eng, eng.scalars()

    assert not exchanging(None)                                       # no process group yet: the single-rank forms
    plain = head(None)
    _, scalars_plain = step("local")
    init_process_group()
    group = torch.distributed.group.WORLD
    assert exchanging(group)
    ungrouped = head(None)                                            # group=None stays on the square kernels whatever is initialised
    grouped = head(group)
    eng, scalars = step("global")
    assert eng.bucketer.exchange and eng._ntxent_group is not None
    torch.save({"backend": torch.distributed.get_backend(), "exchanging": exchanging(group), "plain": plain, "ungrouped": ungrouped,
                "grouped": grouped, "scalars": scalars, "scalars_plain": scalars_plain}, out_path)
else:
    raise SystemExit(f"unknown mode {mode!r}")
if torch.distributed.is_initialized():
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()
