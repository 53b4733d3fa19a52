"""SHA-256 of the outputs of seeded B = 2 forwards of mscoco_uvit_small (with / without mask, bf16 and fp32 residual
stream) and imagenet256_uvit_large: run once per library (PDM_LIB_PATH names another build) and compare the lines.

    python tools/forward_hash.py <tag>
"""
import hashlib
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from panopticdiffusionmodels_amd import configs as C, weights as W
from panopticdiffusionmodels_amd.utils import get_nnet
dev = torch.device("cuda:0")
tag = sys.argv[1]
def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
def net(name):
    cfg = C.nnet_kwargs(name)
    n = get_nnet(**cfg); n.load_state_dict(W.nnet_state_dict(cfg, seed=3, init="random"))
    return n.to(dev).eval()
g = torch.Generator().manual_seed(1)
x = torch.randn(2, 4, 32, 32, generator=g); t = torch.rand(2, generator=g) * 999 + 1
ctx = torch.randn(2, 77, 768, generator=g); mt = torch.randn(2, 8, 32, 32, generator=g)
y = torch.tensor([5, 1000])
with torch.no_grad():
    n = net("mscoco_uvit_small")
    eps, pm = n(x.to(dev), t.to(dev), ctx.to(dev), mask_token=mt.to(dev))
    print(tag, "mscoco_uvit_small with mask   eps", sha(eps), "pred_mask", sha(pm))
    eps = n(x.to(dev), t.to(dev), ctx.to(dev))
    print(tag, "mscoco_uvit_small without mask eps", sha(eps))
    n.set_residual("fp32")
    eps, pm = n(x.to(dev), t.to(dev), ctx.to(dev), mask_token=mt.to(dev))
    print(tag, "mscoco_uvit_small with mask, residual fp32 eps", sha(eps), "pred_mask", sha(pm))
    del n
    n = net("imagenet256_uvit_large")
    eps = n(x.to(dev), t.to(dev), y.to(dev))
    print(tag, "imagenet256_uvit_large         eps", sha(eps))
print(tag, "library:", "the build PDM_LIB_PATH names" if os.environ.get("PDM_LIB_PATH") else "the in-tree build")
