"""Cross-implementation checkpoint parity, direction engine -> reference.

tests/golden/engine_checkpoint_00000003.pth was written on an MI355X by the drop-in CLI's save_checkpoint after three engine
steps (tests/test_gpu_parity.py::test_engine_written_checkpoint_payload, from ckpt_tiny.npz's initial state and batches);
engine_step4.json / engine_student_after_step4.pth hold the engine's step 4 after that point.  ckpt_xref.npz holds what the
REFERENCE's own load_checkpoint (scripts/phase5_big_run.py:1128-1193) restores from that file into reference modules + a stock
torch.optim.AdamW, and the step 4 it takes from there in its loop order (tests/golden/make_golden.py::ckpt_xref).

Here the same file is restored the way that loader does it -- torch.load, the state dicts, the AdamW state_dict into a stock
torch.optim.AdamW, the DINO centre -- into the CPU oracle, which takes step 4 with that optimiser; the restored state and step 4
must match the reference's, and the engine's step 4 must land where the reference's did."""
import json
import os

import pytest
import torch

from conftest import GOLDEN, load_golden, sub, t
from oracle import dinox_oracle as O

CKPT = os.path.join(GOLDEN, "engine_checkpoint_00000003.pth")


def _close_params(got: dict, want: dict, key_bias_atol: float, what: str) -> None:
    for k, v in want.items():
        # (key bias: numerically-zero gradient, Adam moves it by +-lr with a round-off sign -> bounded by steps x lr)
        assert torch.allclose(got[k], v, rtol=1e-3, atol=key_bias_atol if k.endswith("attn.qkv.bias") else 2e-5), f"{what}: {k}"


def test_engine_written_checkpoint_resumes_in_the_reference():
    g = load_golden("ckpt_tiny.npz")
    ref = load_golden("ckpt_xref.npz")
    lr, min_lr, warm, max_steps, wd, ema, ts, tt, cm, gw = [float(v) for v in g["hp"]]
    cfg = O.VitCfg(img_size=28, patch=14, dim=32, depth=2, heads=2, mlp_ratio=4.0, scale_aware=True, out_dim=64)
    payload = torch.load(CKPT, map_location="cpu", weights_only=False)        # as the reference's load_checkpoint reads it
    assert int(payload["step"]) == 3 and payload["config"]["model"]["dim"] == 32 and payload["config"]["scale_aware"] is True
    names = list(O.param_shapes(cfg))                                          # the reference's named_parameters() order
    assert set(payload["student"]) == set(names) and set(payload["teacher"]) == set(names)
    params = [torch.nn.Parameter(payload["student"][k].detach().clone().float()) for k in names]
    opt = torch.optim.AdamW(params, lr=lr, weight_decay=wd)
    opt.load_state_dict(payload["opt"])                                        # the reference's :1168
    assert float(opt.state_dict()["state"][0]["step"]) == 3.0 == float(ref["adam_step3"][0])
    student = dict(zip(names, params))
    teacher = {k: payload["teacher"][k].detach().clone().float() for k in names}
    center = payload["dino_loss"]["center"].detach().clone().float()
    # the restored state is the reference's own state after the same three steps (engine steps == reference steps, 1e-3)
    _close_params(student, sub(g, "student3"), 3.1e-3, "restored student vs the reference's uninterrupted run")
    assert torch.allclose(center, t(g["center3"]), rtol=1e-4, atol=1e-7)
    # ... and exactly what the reference's loader restores from this file
    for k, v in sub(ref, "student3").items():
        assert torch.equal(student[k].detach(), v), k
    for k, v in sub(ref, "teacher3").items():
        assert torch.equal(teacher[k], v), k
    assert torch.equal(center, t(ref["center3"]))
    # step 4 in the reference's loop order (:1692-1802): oracle forward / losses / backward, the stock AdamW restored above
    st = O.TrainState(cfg=cfg, student={k: p.detach() for k, p in student.items()}, teacher=teacher, center=center)
    hp = O.HyperParams(lr=lr, min_lr=min_lr, warmup_steps=int(warm), max_steps=int(max_steps), weight_decay=wd, ema=ema,
                       teacher_temp=tt, student_temp=ts, center_momentum=cm, gram_weight=gw)
    cur_lr = O.get_lr(3, int(max_steps), int(warm), lr, min_lr)
    for pg in opt.param_groups:
        pg["lr"] = cur_lr
    loss, _, _, grads, _, present = O.losses_and_grads(st, t(g["batch3"]), t(g["spacing3"]), hp)
    for k, p in student.items():
        p.grad = grads[k] if present[k] else None
    gn = O.grad_norm({k: v for k, v in grads.items() if present[k]})
    opt.step()
    after = {k: p.detach() for k, p in student.items()}
    ref_loss4, ref_gn4, ref_lr4 = (float(v) for v in ref["step4"])
    assert float(loss) == pytest.approx(ref_loss4, rel=1e-3)
    assert gn == pytest.approx(ref_gn4, rel=1e-3)
    assert cur_lr == pytest.approx(ref_lr4, rel=1e-12)
    _close_params(after, sub(ref, "student4"), 1.1e-3, "oracle step 4 vs the reference's step 4")
    # the engine's step 4 from the same point lands where the reference's does
    eng = json.load(open(os.path.join(GOLDEN, "engine_step4.json")))
    for got, want in ((eng["loss4"], ref_loss4), (eng["grad_norm4"], ref_gn4), (float(loss), eng["loss4"]), (gn, eng["grad_norm4"])):
        assert got == pytest.approx(want, rel=1e-3)
    assert eng["lr4"] == pytest.approx(ref_lr4, rel=1e-12)
    eng_after = torch.load(os.path.join(GOLDEN, "engine_student_after_step4.pth"), map_location="cpu", weights_only=True)
    _close_params(eng_after, sub(ref, "student4"), 1.1e-3, "engine step 4 vs the reference's step 4")
    _close_params(eng_after, after, 1.1e-3, "engine step 4 vs the oracle's step 4")
