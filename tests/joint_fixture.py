"""Shared by tests/test_t2i_joint.py and tests/test_gpu_t2i_joint.py: the seeded inputs behind
tests/golden/joint_golden.npz (the statements of tests/golden/make_joint_golden.py `inputs`, in the same order), checked
against the checksums the generator stored."""
import os

import numpy as np
import torch

from panopticdiffusionmodels_amd import configs as C
from panopticdiffusionmodels_amd import weights as W

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = ("tiny_t2i_joint", "tiny_t2i_joint64")
FULL = ("mscoco_uvit_small_joint", "mscoco_uvit_large", "mscoco_uvit_small_512_joint")
FWD_SEED, SAMPLE_SEED, EMPTY_SEED = 5, 21, 77


def load():
    return np.load(os.path.join(REPO, "tests", "golden", "joint_golden.npz"))


def rel_l2(a, b):
    a = torch.as_tensor(np.asarray(a.detach().cpu() if torch.is_tensor(a) else a)).double()
    b = torch.as_tensor(np.asarray(b.detach().cpu() if torch.is_tensor(b) else b)).double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _checksum(vals):
    return np.array([float(v.double().sum()) for v in vals] + [float(v.double().abs().sum()) for v in vals])


def _inputs(name, B, seed):
    cfg = C.get_config(name)
    n = cfg["nnet"]
    g = torch.Generator().manual_seed(seed)
    Cc, H, Wd = cfg["z_shape"]
    return {"x": torch.randn(B, Cc, H, Wd, generator=g),
            "t": torch.rand(B, generator=g) * 998.0 + 1.0,
            "context": torch.randn(B, n["num_clip_token"], n["clip_dim"], generator=g),
            "mask_token": torch.randn(B, n.get("num_panoptic_class", 8), H, Wd, generator=g)}


def forward_inputs(golden, name):
    """x, t, context, mask_token of the B = 2 forward of `name`."""
    inp = _inputs(name, 2, FWD_SEED)
    np.testing.assert_allclose(_checksum(inp.values()), golden[f"{name}/in_checksum"], rtol=1e-12, atol=1e-9)
    for k in inp:   # stored for tiny_t2i_joint: the regenerated tensors are the stored ones
        if f"{name}/in_{k}" in golden.files:
            assert np.array_equal(inp[k].numpy(), golden[f"{name}/in_{k}"])
    return inp


def sample_inputs(golden, name):
    """z_init (x), context, mask_init (mask_token) and the empty context of the B = 2, 50-NFE sample of `name`."""
    inp = _inputs(name, 2, SAMPLE_SEED)
    n = C.nnet_kwargs(name)
    g = torch.Generator().manual_seed(EMPTY_SEED)
    inp["empty"] = torch.randn(n["num_clip_token"], n["clip_dim"], generator=g)
    np.testing.assert_allclose(_checksum(inp.values()), golden[f"sample/{name}/in_checksum"], rtol=1e-12, atol=1e-9)
    for k, gk in (("x", "z_init"), ("context", "context"), ("empty", "empty_context"), ("mask_token", "mask_init")):
        if f"sample/{name}/{gk}" in golden.files:
            assert np.array_equal(inp[k].numpy(), golden[f"sample/{name}/{gk}"])
    return inp


def state_dict(golden, name):
    """(nnet kwargs without `name`, the seeded state_dict), checked against the generator's checksums."""
    cfg = C.nnet_kwargs(name)
    sd = W.nnet_state_dict(cfg, seed=11, init="random")
    np.testing.assert_allclose(_checksum(sd.values()), golden[f"{name}/sd_checksum"], rtol=1e-12, atol=1e-9)
    kw = dict(cfg)
    kw.pop("name")
    return kw, sd
