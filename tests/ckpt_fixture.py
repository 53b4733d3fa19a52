"""The reference-written step-3 checkpoint of tiny_uvit_train, rebuilt from tests/golden/ckpt_golden*.npz and
train_golden.npz (tests/golden/make_ckpt_golden.py): shared by tests/test_train_ckpt.py and
tests/test_gpu_train_ckpt.py.  Only recorded data is read; the reference itself is not needed."""
import json
import os

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
NAME = "tiny_uvit_train"


class Fixture:
    """ckpt_golden.npz, ckpt_golden_sq.npz and ckpt_golden_grad.npz behind one mapping (loaded once per process)."""
    _cache = None

    def __init__(self):
        self.parts = [np.load(os.path.join(GOLDEN, f)) for f in ("ckpt_golden.npz", "ckpt_golden_sq.npz",
                                                                 "ckpt_golden_grad.npz")]
        self.tg = np.load(os.path.join(GOLDEN, "train_golden.npz"))
        self.names = [str(k) for k in self["names"]]
        self.group = json.loads(str(self["group_json"]))
        self.sched = json.loads(str(self["sched_json"]))
        self.step = int(self["step_pth"])

    def __getitem__(self, key):
        for p in self.parts:
            if key in p.files:
                return p[key]
        raise KeyError(key)

    @classmethod
    def get(cls):
        if cls._cache is None:
            cls._cache = cls()
        return cls._cache

    def t(self, key):
        return torch.from_numpy(self[key])

    # ---- the reference's step-3 files ------------------------------------------------------------------------
    def nnet_sd(self):
        return {k: torch.from_numpy(self.tg[f"{NAME}/param/{k}"]) for k in self.names}

    def ema_sd(self):
        return {k: torch.from_numpy(self.tg[f"{NAME}/ema/{k}"]) for k in self.names}

    def exp_avg(self):
        return {k: self.t(f"exp_avg/{k}") for k in self.names}

    def exp_avg_sq(self):
        return {k: self.t(f"exp_avg_sq/{k}") for k in self.names}

    def optimizer_sd(self):
        """optimizer.pth as the reference's torch.optim.AdamW wrote it."""
        dt = getattr(torch, str(self["param_step_dtype"]).replace("torch.", ""))
        m, v = self.exp_avg(), self.exp_avg_sq()
        state = {i: {"step": torch.tensor(float(self["param_step"][i]), dtype=dt), "exp_avg": m[k],
                     "exp_avg_sq": v[k]} for i, k in enumerate(self.names)}
        group = dict(self.group)
        group["betas"] = tuple(group["betas"])
        group["params"] = list(range(len(self.names)))
        return {"state": state, "param_groups": [group]}

    def sched_sd(self):
        return dict(self.sched)

    def write_dir(self, path):
        """<path>/ = the directory utils.TrainState.save wrote after three iterations."""
        os.makedirs(path, exist_ok=True)
        torch.save(self.step, os.path.join(path, "step.pth"))
        torch.save(self.nnet_sd(), os.path.join(path, "nnet.pth"))
        torch.save(self.ema_sd(), os.path.join(path, "nnet_ema.pth"))
        torch.save(self.optimizer_sd(), os.path.join(path, "optimizer.pth"))
        torch.save(self.sched_sd(), os.path.join(path, "lr_scheduler.pth"))
        return path


def jsonable(v):
    """Tuples as lists, dict keys as str: the form the fixture's JSON fields have."""
    if isinstance(v, (tuple, list)):
        return [jsonable(x) for x in v]
    if isinstance(v, dict):
        return {str(k): jsonable(x) for k, x in v.items()}
    return v
