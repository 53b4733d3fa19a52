"""The reference's checkpoint directory (utils.TrainState.save / load / resume, utils.py:367-405) as plain functions
over dicts of CPU tensors: no GPU, no trainer.

A checkpoint `<root>/<step>.ckpt/` holds what torch writes for the reference:
  step.pth          the Python int train_state.step
  nnet.pth          nnet.state_dict()      (reference keys, fp32)
  nnet_ema.pth      nnet_ema.state_dict()
  optimizer.pth     torch.optim.AdamW.state_dict(): state[i] = {step, exp_avg, exp_avg_sq}, i the index in
                    nnet.parameters() order; one param group
  lr_scheduler.pth  LambdaLR.state_dict() of utils.customized_lr_scheduler (lr_lambdas: [None])
HipTrainState keeps ONE step counter, so step.pth, every per-parameter `step` and the scheduler's last_epoch must
agree (they do in every directory the reference's loop writes: optimizer.step(), lr_scheduler.step() and
train_state.step += 1 run together, train_ldm_discrete.py:159-175).
"""
import os

import torch

from . import weights

FILES = ("step.pth", "nnet.pth", "nnet_ema.pth", "optimizer.pth", "lr_scheduler.pth")


def param_order(nnet_kwargs):
    """[(name, shape)] in the reference's nnet.parameters() order (the index torch.optim keys its state by): the
    modules' registration order, which is the order of the state_dict spec (weights.py)."""
    kw = dict(nnet_kwargs)
    name = kw.pop("name", "uvit")
    if name == "uvit":
        spec = weights.uvit_spec(**kw)
    elif name == "uvit_t2i":
        spec = weights.uvit_t2i_spec(**kw)
    else:
        raise NotImplementedError(name)
    return [(k, tuple(shape)) for k, shape, _ in spec]


def customized_factor(step, warmup_steps=-1):
    """utils.customized_lr_scheduler's lambda (utils.py:321-325)."""
    return min(step / warmup_steps, 1) if warmup_steps > 0 else 1


def _throwaway(hyper):
    """A torch.optim.AdamW over an empty CPU tensor under LambdaLR, with the trainer's hyper-parameters: the source of
    the param group / scheduler dict in the form this torch version writes."""
    from torch.optim.lr_scheduler import LambdaLR
    opt = torch.optim.AdamW([torch.empty(0)], lr=float(hyper["lr"]), betas=tuple(float(b) for b in hyper["betas"]),
                            eps=float(hyper.get("eps", 1e-8)), weight_decay=float(hyper["weight_decay"]))
    return opt, LambdaLR(opt, lambda step: 1)


def optimizer_state_dict(order, exp_avg, exp_avg_sq, step, hyper, warmup_steps=-1, stateless=()):
    """torch.optim.AdamW.state_dict() after `step` optimizer steps.  order: param_order(); exp_avg / exp_avg_sq:
    name -> CPU tensor; hyper: dict(lr = the base rate, betas, eps, weight_decay); stateless: names of parameters that
    never had a gradient (no entry in `state`).  No step taken yet: an empty `state`, as torch's."""
    opt, _ = _throwaway(hyper)
    group = dict(opt.state_dict()["param_groups"][0])
    base = float(hyper["lr"])
    group["lr"] = base * customized_factor(step, warmup_steps)
    group["initial_lr"] = base
    group["params"] = list(range(len(order)))
    state = {}
    if step > 0:
        for i, (name, shape) in enumerate(order):
            if name in stateless:
                continue
            state[i] = {"step": torch.tensor(float(step)),
                        "exp_avg": exp_avg[name].detach().to("cpu", torch.float32).reshape(shape).clone(),
                        "exp_avg_sq": exp_avg_sq[name].detach().to("cpu", torch.float32).reshape(shape).clone()}
    return {"state": state, "param_groups": [group]}


def lr_scheduler_state_dict(step, hyper, warmup_steps=-1):
    """LambdaLR.state_dict() of utils.customized_lr_scheduler after `step` lr_scheduler.step() calls."""
    _, sched = _throwaway(hyper)
    sd = dict(sched.state_dict())
    base = float(hyper["lr"])
    sd["base_lrs"] = [base]
    sd["last_epoch"] = int(step)
    sd["_step_count"] = int(step) + 1
    sd["_last_lr"] = [base * customized_factor(step, warmup_steps)]
    sd["lr_lambdas"] = [None]
    return sd


def read_optimizer_state_dict(sd, order, stateless=()):
    """The way back: (exp_avg, exp_avg_sq, step, hyper).  exp_avg / exp_avg_sq: name -> fp32 CPU tensor for every
    parameter with state; step: the one per-parameter step (None for an empty state); hyper: dict(lr = initial_lr,
    betas, eps, weight_decay) from the param group, as optimizer.load_state_dict takes them from the file.
    ValueError for more than one param group, a parameter count / shape mismatch, per-parameter steps that differ, or
    state for a parameter in `stateless`."""
    groups = sd["param_groups"]
    if len(groups) != 1:
        raise ValueError(f"optimizer state_dict: one param group expected, got {len(groups)}")
    g = groups[0]
    if len(g["params"]) != len(order):
        raise ValueError(f"optimizer state_dict: {len(g['params'])} parameters, the network has {len(order)}")
    index = {pid: i for i, pid in enumerate(g["params"])}
    exp_avg, exp_avg_sq, steps = {}, {}, set()
    for pid, st in sd["state"].items():
        if pid not in index:
            raise ValueError(f"optimizer state_dict: state for unknown parameter id {pid}")
        name, shape = order[index[pid]]
        if name in stateless:
            raise ValueError(f"optimizer state_dict: state for {name}, a parameter the forward never uses "
                             f"(it never has a gradient, so torch.optim keeps no state for it)")
        for key, dst in (("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq)):
            t = torch.as_tensor(st[key]).detach().to("cpu", torch.float32)
            if tuple(t.shape) != tuple(shape):
                raise ValueError(f"optimizer state_dict: {key} of {name} has shape {tuple(t.shape)}, not {shape}")
            dst[name] = t
        steps.add(float(st["step"]))
    if len(steps) > 1:
        raise ValueError(f"optimizer state_dict: per-parameter steps differ: {sorted(steps)} (HipTrainState keeps one "
                         f"step counter)")
    step = None
    if steps:
        s = steps.pop()
        if s != int(s):
            raise ValueError(f"optimizer state_dict: non-integer step {s}")
        step = int(s)
        have = set(exp_avg)
        lacking = [n for n, _ in order if n not in stateless and n not in have]
        if lacking:
            raise ValueError(f"optimizer state_dict: no state for {lacking[:5]} (HipTrainState steps every used "
                             f"parameter together)")
    hyper = dict(lr=float(g.get("initial_lr", g["lr"])), betas=tuple(float(b) for b in g["betas"]),
                 eps=float(g["eps"]), weight_decay=float(g["weight_decay"]))
    return exp_avg, exp_avg_sq, step, hyper


def read_lr_scheduler_state_dict(sd):
    """(last_epoch, base_lr) of a LambdaLR state_dict with one param group."""
    if len(sd["base_lrs"]) != 1:
        raise ValueError(f"lr_scheduler state_dict: one base_lr expected, got {len(sd['base_lrs'])}")
    return int(sd["last_epoch"]), float(sd["base_lrs"][0])


def check_steps(step, param_step, last_epoch):
    """The single-counter rule: step.pth, the per-parameter optimizer step (None: empty state, i.e. 0) and the
    scheduler's last_epoch must agree."""
    ps = 0 if param_step is None else param_step
    if not (int(step) == int(ps) == int(last_epoch)):
        raise ValueError(f"checkpoint steps disagree: step.pth = {step}, optimizer per-parameter step = {param_step}, "
                         f"lr_scheduler last_epoch = {last_epoch} (HipTrainState keeps one step counter)")
    return int(step)


def resume_path(ckpt_root, step=None):
    """utils.TrainState.resume's choice of directory (utils.py:387-405): None for a missing root or one without any
    '*.ckpt'; the largest numeric <step>.ckpt, or best.ckpt when the first entry listed is not numeric; `step` given:
    <step>.ckpt."""
    if not os.path.exists(ckpt_root):
        return None
    if step is None:
        ckpts = [x for x in os.listdir(ckpt_root) if ".ckpt" in x]
        if not ckpts:
            return None
        if not ckpts[0].split(".")[0].isnumeric():
            return os.path.join(ckpt_root, "best.ckpt")
        step = max(int(x.split(".")[0]) for x in ckpts)
    return os.path.join(ckpt_root, f"{step}.ckpt")


def write_dir(path, step, nnet_sd, ema_sd, opt_sd, sched_sd):
    """utils.TrainState.save (utils.py:367-372)."""
    os.makedirs(path, exist_ok=True)
    torch.save(int(step), os.path.join(path, "step.pth"))
    torch.save(nnet_sd, os.path.join(path, "nnet.pth"))
    torch.save(ema_sd, os.path.join(path, "nnet_ema.pth"))
    torch.save(opt_sd, os.path.join(path, "optimizer.pth"))
    torch.save(sched_sd, os.path.join(path, "lr_scheduler.pth"))


def read_dir(path):
    """(step, nnet_sd, ema_sd, opt_sd, sched_sd) with plain torch.load(map_location='cpu') (utils.py:374-385)."""
    out = [torch.load(os.path.join(path, "step.pth"))]
    for f in FILES[1:]:
        out.append(torch.load(os.path.join(path, f), map_location="cpu"))
    return tuple(out)


__all__ = ["param_order", "optimizer_state_dict", "lr_scheduler_state_dict", "read_optimizer_state_dict",
           "read_lr_scheduler_state_dict", "check_steps", "resume_path", "write_dir", "read_dir", "FILES"]
