"""Forward modes of the one block runner / stack walk (csrc/capi.hip run_block, run_stack, t2i_two_stream16 / 32) that
no other test reaches, each against the fp32 CPU oracle (oracle/uvit_ref.py) at the standing bounds: rel-L2 < 2e-2 for
bf16 operands (test_fullsize_golden.py), test_gpu_fp8.py's TOL_FP8_FWD for the MXFP8 precisions.

* an MXFP8 net without long skips (skip=False): what each block leaves for the next one differs there (no bf16 copy
  on the fp32 stream, the MXFP8 output after the mid block and the out-blocks), at the smallest admissible shape
  (embed_dim 128, mlp hidden 512, depth 2);
* the two-stream t2i forward on the fp32 residual stream at tiny_t2i, with and without use_ground_truth;
* tiny_t2i at depth 1 (no in- / out-blocks: the mid layer is the first one, so its mask-stream input takes the image
  rows of the token assembly) on the bf16 stream."""
import pytest
import torch

from oracle import uvit_ref
from panopticdiffusionmodels_amd import configs as C
from panopticdiffusionmodels_amd import weights as W
from panopticdiffusionmodels_amd.utils import get_nnet

pytestmark = pytest.mark.gpu

TOL_BF16 = 2e-2
TOL_FP8_FWD = {"fp8": 6e-2, "fp8-all": 8e-2}   # test_gpu_fp8.py


def rel(a, b):
    a = torch.as_tensor(a).double().cpu()
    b = torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _net(cfg, dev):
    sd = W.nnet_state_dict(cfg, seed=3, init="random")
    net = get_nnet(**cfg)
    net.load_state_dict(sd)
    kw = dict(cfg)
    kw.pop("name")
    return net.to(dev).eval(), sd, kw


def _inputs(B=2, seed=1):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 4, 16, 16, generator=g)
    t = torch.rand(B, generator=g) * 999 + 1
    ctx = torch.randn(B, 5, 64, generator=g)
    mt = torch.randn(B, 8, 16, 16, generator=g)
    return x, t, ctx, mt


@pytest.fixture(scope="module")
def noskip(dev):
    cfg = dict(name="uvit", img_size=16, patch_size=2, in_chans=4, embed_dim=128, depth=2, num_heads=2, mlp_ratio=4,
               qkv_bias=False, mlp_time_embed=False, num_classes=11, skip=False)
    net, sd, kw = _net(cfg, dev)
    x, t, _, _ = _inputs()
    y = torch.tensor([3, 10])
    with torch.no_grad():
        ref = uvit_ref.uvit_forward(sd, kw, x, t, y)
    return net, (x.to(dev), t.to(dev), y.to(dev)), ref


@pytest.mark.parametrize("residual", ["bf16", "fp32"])
@pytest.mark.parametrize("precision", ["fp8", "fp8-all"])
def test_fp8_forward_without_long_skips_vs_oracle(noskip, precision, residual):
    net, inp, ref = noskip
    with torch.no_grad():
        eps = net.set_residual(residual).set_precision(precision)(*inp).cpu()
    assert torch.isfinite(eps).all()
    err = rel(eps, ref)
    print(f"skip=False {precision} (residual {residual}) rel-L2 {err:.3e}")
    assert err < TOL_FP8_FWD[precision], err


@pytest.fixture(scope="module")
def tiny_t2i(dev):
    net, sd, kw = _net(C.nnet_kwargs("tiny_t2i"), dev)
    return net.set_residual("fp32"), sd, kw


@pytest.mark.parametrize("use_ground_truth", [False, True])
def test_t2i_two_stream_fp32_residual_vs_oracle(dev, tiny_t2i, use_ground_truth):
    net, sd, kw = tiny_t2i
    x, t, ctx, mt = _inputs(seed=2)
    with torch.no_grad():
        eps, y = net(x.to(dev), t.to(dev), ctx.to(dev), mask_token=mt.to(dev), use_ground_truth=use_ground_truth)
        ref_eps, ref_y = uvit_ref.uvit_t2i_forward(sd, kw, x, t, ctx, mask_token=mt, use_ground_truth=use_ground_truth)
    assert torch.isfinite(eps).all()
    print(f"tiny_t2i fp32 residual, use_ground_truth={use_ground_truth}: eps rel-L2 {rel(eps, ref_eps):.3e}")
    assert rel(eps, ref_eps) < TOL_BF16
    if use_ground_truth:
        assert torch.equal(y.cpu(), mt)
    else:
        print(f"  pred_mask rel-L2 {rel(y, ref_y):.3e}")
        assert rel(y, ref_y) < TOL_BF16


def test_t2i_two_stream_depth_1_vs_oracle(dev):
    net, sd, kw = _net(dict(C.nnet_kwargs("tiny_t2i"), depth=1), dev)
    x, t, ctx, mt = _inputs(seed=4)
    with torch.no_grad():
        eps, pm = net(x.to(dev), t.to(dev), ctx.to(dev), mask_token=mt.to(dev))
        ref_eps, ref_pm = uvit_ref.uvit_t2i_forward(sd, kw, x, t, ctx, mask_token=mt)
    print(f"tiny_t2i depth 1: eps rel-L2 {rel(eps, ref_eps):.3e}, pred_mask rel-L2 {rel(pm, ref_pm):.3e}")
    assert torch.isfinite(eps).all() and torch.isfinite(pm).all()
    assert rel(eps, ref_eps) < TOL_BF16
    assert rel(pm, ref_pm) < TOL_BF16
