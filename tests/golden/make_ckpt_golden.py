"""Generate tests/golden/ckpt_golden*.npz: the REFERENCE's own checkpoint of its training loop on tiny_uvit_train
(build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_ckpt_golden.py [/root/reference]

Five iterations of the loop make_train_golden.py runs for three (same batch, same seed pattern (100 + i, 200 + i)), with
the reference's utils.TrainState and utils.ema executed from its source (`ast`, as make_train_golden._ref_defs; `os`
is the real module, `logging` a stub).  After iteration index 2 (three optimizer steps) the parameters and the EMA
are asserted bit-equal to train_golden.npz -- they are not stored again -- and the reference's own TrainState.save
writes a checkpoint directory that is read back with plain torch.load.  Stored (data only):
  ckpt_golden.npz       names in named_parameters() order (also of tiny_uvit_train_uncond and of the t2i net of
                        tiny_t2i_train, with the t2i names that have no optimizer state after one iteration), exp_avg
                        per name, the per-parameter step, step.pth, the param group and the scalar fields of the
                        LambdaLR dict (JSON), the draws / losses / LRs of iterations 3 and 4, and sketches (norm + 8
                        seeded Gaussian projections, make_train_h_golden.sketch) of the parameters and EMA after
                        iteration 5
  ckpt_golden_sq.npz    exp_avg_sq per name
  ckpt_golden_grad.npz  the gradients of iteration 3
(three files so that each stays below the 1 MiB limit for a committed file).  Nothing here is imported by the
product or run on the GPU box.
"""
import json
import os
import random
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import C, W, _import_reference, _np  # noqa: E402
from make_train_golden import SEEDS as SEEDS3, _ref_defs, batch  # noqa: E402
from make_train_h_golden import sketch  # noqa: E402
import make_t2i_train_golden as T2I  # noqa: E402

ITERS = 5
SEEDS = [(100 + i, 200 + i) for i in range(ITERS)]
assert SEEDS[:len(SEEDS3)] == SEEDS3
NAME = "tiny_uvit_train"


def _jsonable(v):
    if isinstance(v, (tuple, list)):
        return [_jsonable(x) for x in v]
    if isinstance(v, dict):
        return {str(k): _jsonable(x) for k, x in v.items()}
    assert v is None or isinstance(v, (bool, int, float, str)), type(v)
    return v


def t2i_names(ref, mods):
    """named_parameters() order of the t2i net and the names without optimizer state after one reference iteration."""
    uvit_t2i = mods[1]
    ns = {"torch": torch, "np": np, "nn": torch.nn, "random": random, "p_uncond": 0.0, "use_panoptic": True,
          "use_ground_truth": False, "use_twophases": False}
    uns = _ref_defs(os.path.join(ref, "utils.py"), {"int2bits"}, {"torch": torch, "np": np})
    ns["utils"] = types.SimpleNamespace(int2bits=uns["int2bits"])
    _ref_defs(os.path.join(ref, "train_t2i_discrete.py"),
              {"stable_diffusion_beta_schedule", "get_skip", "stp", "mos", "Schedule", "LSimple"}, ns)
    full = C.get_config(T2I.NAME)
    cfg = full["nnet"]
    kw = dict(cfg)
    kw.pop("name")
    net = uvit_t2i.UViT(**kw)
    net.load_state_dict(W.nnet_state_dict(cfg, seed=11, init="random"))
    net.train()
    opt = full["optimizer"]
    optimizer = torch.optim.AdamW(net.parameters(), lr=opt["lr"], weight_decay=opt["weight_decay"],
                                  betas=tuple(opt["betas"]))
    x0, ctx, pan = T2I.batch()
    schedule = ns["Schedule"](ns["stable_diffusion_beta_schedule"]())
    np.random.seed(T2I.SEEDS[0][0])
    torch.manual_seed(T2I.SEEDS[0][1])
    random.seed(0)
    loss_eps, loss_mask = ns["LSimple"](x0, net, schedule, panoptic=pan, context=ctx)
    (loss_eps.mean() + loss_mask.mean()).backward()
    optimizer.step()
    names = [k for k, _ in net.named_parameters()]
    assert [id(p) for p in net.parameters()] == [id(p) for _, p in net.named_parameters()]
    state = optimizer.state_dict()["state"]
    return names, [k for i, k in enumerate(names) if i not in state]


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    mods = _import_reference(ref)
    uvit = mods[0]
    ns = {"torch": torch, "np": np, "nn": torch.nn, "os": os,
          "logging": types.SimpleNamespace(info=lambda *a, **k: None)}
    _ref_defs(os.path.join(ref, "train_ldm_discrete.py"),
              {"stable_diffusion_beta_schedule", "get_skip", "stp", "mos", "Schedule", "LSimple"}, ns)
    _ref_defs(os.path.join(ref, "utils.py"), {"customized_lr_scheduler", "ema", "TrainState"}, ns)
    tg = np.load(os.path.join(HERE, "train_golden.npz"))
    full = C.get_config(NAME)
    cfg = full["nnet"]
    sd = W.nnet_state_dict(cfg, seed=11, init="random")
    kw = dict(cfg)
    kw.pop("name")
    net = uvit.UViT(**kw)
    net.load_state_dict(sd)
    net_ema = uvit.UViT(**kw)
    net_ema.load_state_dict(sd)
    net.train()
    opt = full["optimizer"]
    optimizer = torch.optim.AdamW(net.parameters(), lr=opt["lr"], weight_decay=opt["weight_decay"],
                                  betas=tuple(opt["betas"]))
    sched = ns["customized_lr_scheduler"](optimizer, warmup_steps=full["lr_scheduler"]["warmup_steps"])
    train_state = ns["TrainState"](optimizer=optimizer, lr_scheduler=sched, step=0, nnet=net, nnet_ema=net_ema)
    x0, y = batch(NAME)
    schedule = ns["Schedule"](ns["stable_diffusion_beta_schedule"]())
    names = [k for k, _ in net.named_parameters()]
    assert [id(p) for p in net.parameters()] == [id(p) for _, p in net.named_parameters()]
    out, out_sq, out_grad = {"names": np.array(names)}, {}, {}
    for i, (nps, ts) in enumerate(SEEDS):
        optimizer.zero_grad()
        np.random.seed(nps)
        torch.manual_seed(ts)
        loss = ns["LSimple"](x0, net, schedule, y=y)
        if i >= 3:
            np.random.seed(nps)
            torch.manual_seed(ts)
            n, eps, xn = schedule.sample(x0)   # the same draw, recorded
            out[f"it{i}_t"] = _np(n.float())
            out[f"it{i}_eps"] = _np(eps)
            out[f"it{i}_xt"] = _np(xn)
            out[f"it{i}_loss"] = _np(loss)
            out[f"it{i}_lr"] = np.array(optimizer.param_groups[0]["lr"])
        loss.mean().backward()
        if i == 3:
            for k, p in net.named_parameters():
                out_grad[f"grad/{k}"] = _np(p.grad if p.grad is not None else torch.zeros_like(p))
        optimizer.step()
        sched.step()
        train_state.ema_update(full["train"]["ema_rate"])
        train_state.step += 1
        if i == 2:
            for k, p in net.named_parameters():
                assert np.array_equal(_np(p), tg[f"{NAME}/param/{k}"]), f"step-3 parameter {k} differs from train_golden"
            for k, p in net_ema.named_parameters():
                assert np.array_equal(_np(p), tg[f"{NAME}/ema/{k}"]), f"step-3 EMA {k} differs from train_golden"
            with tempfile.TemporaryDirectory() as tmp:
                path = os.path.join(tmp, "3.ckpt")
                train_state.save(path)
                assert sorted(os.listdir(path)) == ["lr_scheduler.pth", "nnet.pth", "nnet_ema.pth", "optimizer.pth",
                                                    "step.pth"]
                step = torch.load(os.path.join(path, "step.pth"))
                nsd = torch.load(os.path.join(path, "nnet.pth"), map_location="cpu")
                osd = torch.load(os.path.join(path, "optimizer.pth"), map_location="cpu")
                ssd = torch.load(os.path.join(path, "lr_scheduler.pth"), map_location="cpu")
            assert list(nsd) == names   # no buffers: the state_dict is the parameters, in their order
            out["step_pth"] = np.array(step)
            assert sorted(osd["state"]) == list(range(len(names))) and len(osd["param_groups"]) == 1
            out["param_step"] = np.array([float(osd["state"][j]["step"]) for j in range(len(names))])
            out["param_step_dtype"] = np.array(str(osd["state"][0]["step"].dtype))
            for j, k in enumerate(names):
                out[f"exp_avg/{k}"] = _np(osd["state"][j]["exp_avg"])
                out_sq[f"exp_avg_sq/{k}"] = _np(osd["state"][j]["exp_avg_sq"])
            group = dict(osd["param_groups"][0])
            assert group.pop("params") == list(range(len(names)))
            out["group_json"] = np.array(json.dumps(_jsonable(group)))
            out["sched_json"] = np.array(json.dumps(_jsonable(ssd)))
    for k, p in net.named_parameters():
        out[f"psk5/{k}"] = sketch(k, p.detach())
    for k, p in net_ema.named_parameters():
        out[f"esk5/{k}"] = sketch(k, p.detach())
    ucfg = dict(C.get_config("tiny_uvit_train_uncond")["nnet"])
    ucfg.pop("name")
    out["uncond_names"] = np.array([k for k, _ in uvit.UViT(**ucfg).named_parameters()])
    tn, stateless = t2i_names(ref, mods)
    out["t2i_names"] = np.array(tn)
    out["t2i_stateless"] = np.array(stateless)
    for fname, d in (("ckpt_golden.npz", out), ("ckpt_golden_sq.npz", out_sq), ("ckpt_golden_grad.npz", out_grad)):
        path = os.path.join(HERE, fname)
        np.savez_compressed(path, **d)
        size = os.path.getsize(path)
        print(f"wrote {path}: {len(d)} arrays, {size / 1e6:.2f} MB")
        assert size < (1 << 20), f"{fname} is above the 1 MiB limit for a committed file"


if __name__ == "__main__":
    main()
