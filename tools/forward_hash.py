"""SHA-256 of the outputs of seeded forwards over every mode of the forward drivers (csrc/capi.hip): class-conditional
and unconditional nets, MXFP8 nets with and without long skips, the two-stream and the joint t2i nets with / without
mask tokens and use_ground_truth, each on the bf16 and on the fp32 residual stream.  Run once per library
(PDM_LIB_PATH names another build) and compare the lines.

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
RESIDUALS = ("bf16", "fp32")


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def net(cfg):
    n = get_nnet(**cfg)
    n.load_state_dict(W.nnet_state_dict(cfg, seed=3, init="random"))
    return n.to(dev).eval()


def inputs(cfg, B):
    g = torch.Generator().manual_seed(1)
    s, c = cfg["img_size"], cfg["in_chans"]
    x = torch.randn(B, c, s, s, generator=g)
    t = torch.rand(B, generator=g) * 999 + 1
    ctx = torch.randn(B, cfg.get("num_clip_token", 1), cfg.get("clip_dim", 1), generator=g)
    mt = torch.randn(B, cfg.get("num_panoptic_class", 8), s, s, generator=g)
    y = torch.randint(0, max(cfg.get("num_classes", 0), 1), (B,), generator=g)
    return [v.to(dev) for v in (x, t, ctx, mt, y)]


def class_cond(label, cfg, B, precisions=("bf16",)):
    n = net(cfg)
    x, t, _, _, y = inputs(cfg, B)
    for p in precisions:
        for r in RESIDUALS:
            eps = n.set_residual(r).set_precision(p)(x, t, y if cfg["num_classes"] > 0 else None)
            print(tag, f"{label} B={B} {p} residual={r} eps", sha(eps))


def t2i(label, cfg, B=2):
    n = net(cfg)
    x, t, ctx, mt, _ = inputs(cfg, B)
    for r in RESIDUALS:
        n.set_residual(r)
        print(tag, f"{label} residual={r} no mask eps", sha(n(x, t, ctx)))
        eps, pm = n(x, t, ctx, mask_token=mt)
        print(tag, f"{label} residual={r} mask eps", sha(eps), "pred_mask", sha(pm))
        eps, _ = n(x, t, ctx, mask_token=mt, use_ground_truth=True)
        print(tag, f"{label} residual={r} mask, use_ground_truth eps", sha(eps))


SMALL8 = dict(name="uvit", img_size=16, patch_size=2, in_chans=4, embed_dim=128, depth=2, num_heads=2, mlp_ratio=4,
              qkv_bias=False, mlp_time_embed=False, num_classes=11)   # the smallest shape the MXFP8 path admits
with torch.no_grad():
    for name in ("tiny_uvit_cond", "tiny_uvit_uncond"):
        class_cond(name, C.nnet_kwargs(name), 2)
    for B in (2, 100):   # 100 rows: the bench's persistent-kernel policy
        class_cond("imagenet256_uvit_large", C.nnet_kwargs("imagenet256_uvit_large"), B)
    for name, cfg in (("small8", SMALL8), ("imagenet256_uvit_huge", C.nnet_kwargs("imagenet256_uvit_huge")),
                      ("imagenet512_uvit_huge", C.nnet_kwargs("imagenet512_uvit_huge"))):
        for skip in (True, False):
            class_cond(f"{name} skip={skip}", dict(cfg, skip=skip), 2, precisions=("fp8", "fp8-all"))
    for name in ("tiny_t2i", "mscoco_uvit_small", "tiny_t2i_joint", "tiny_t2i_joint64"):
        t2i(name, C.nnet_kwargs(name))
    t2i("tiny_t2i depth=1", dict(C.nnet_kwargs("tiny_t2i"), depth=1))
print(tag, "library:", "the build PDM_LIB_PATH names" if os.environ.get("PDM_LIB_PATH") else "the in-tree build")
