"""The joint image+mask sequence of the panoptic t2i U-ViT (`enable_panoptic=True, separate=False`) on the HIP path,
against the reference's own outputs (tests/golden/joint_golden.npz) and the fp32 oracle.

Tolerances (as tests/test_gpu_t2i.py / tests/test_gpu_configs.py use them for the separate layout): bf16
forward vs reference or oracle rel-L2 <= 2e-2, final latent after 50 NFE <= 1e-2, pred_mask <= 2e-2, graph vs eager
bit-exact, batch-shard invariance <= 1e-6."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import joint_fixture as J  # noqa: E402

from oracle import uvit_ref  # noqa: E402
from panopticdiffusionmodels_amd import configs as C  # noqa: E402
from panopticdiffusionmodels_amd import weights as W  # noqa: E402
from panopticdiffusionmodels_amd.sampler import T2ISampler  # noqa: E402
from panopticdiffusionmodels_amd.utils import get_nnet  # noqa: E402

pytestmark = pytest.mark.gpu
rel = J.rel_l2


@pytest.fixture(scope="module")
def jg():
    return J.load()


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


_nets = {}


def _net(jg, name, dev, residual="bf16"):
    """One module per config for the whole file (seed 11, the fixture's weights), in the asked residual mode."""
    if name not in _nets:
        kw, sd = J.state_dict(jg, name)
        n = get_nnet(name="uvit_t2i", **kw)
        n.load_state_dict(sd)
        _nets[name] = n.to(dev).eval()
    n = _nets[name]
    if n.residual != residual:
        n.set_residual(residual)
    return n


def _cuda(inp, dev):
    return {k: v.to(dev) for k, v in inp.items()}


@pytest.mark.parametrize("residual", ["bf16", "fp32"])
@pytest.mark.parametrize("name", J.TINY)
def test_tiny_forwards_vs_reference(jg, dev, name, residual):
    net = _net(jg, name, dev, residual)
    i = _cuda(J.forward_inputs(jg, name), dev)
    with torch.no_grad():
        eps, pm = net(i["x"], i["t"], i["context"], mask_token=i["mask_token"])
        eps_n = net(i["x"], i["t"], i["context"])
        eps_g, y = net(i["x"], i["t"], i["context"], mask_token=i["mask_token"], use_ground_truth=True)
    errs = dict(eps_mask=rel(eps, jg[f"{name}/eps_mask"]), pred_mask=rel(pm, jg[f"{name}/pred_mask"]),
                eps_nomask=rel(eps_n, jg[f"{name}/eps_nomask"]), eps_gt=rel(eps_g, jg[f"{name}/eps_gt"]))
    print(name, residual, errs)
    assert all(e < 2e-2 for e in errs.values()), errs
    assert torch.equal(y, i["mask_token"])


@pytest.mark.parametrize("residual", ["bf16", "fp32"])
@pytest.mark.parametrize("name", J.TINY)
def test_nothing_written_outside_the_outputs(jg, dev, name, residual):
    """out= / mask_out= as views into NaN-filled tensors: the guard samples on both sides stay NaN, every element
    inside is written, and the values are those of the forward that allocates its own outputs."""
    net = _net(jg, name, dev, residual)
    i = _cuda(J.forward_inputs(jg, name), dev)
    B, Cc, S = i["x"].shape[0], i["x"].shape[1], i["x"].shape[2]
    K = i["mask_token"].shape[1]
    for mt, gt in ((i["mask_token"], False), (None, False), (i["mask_token"], True)):
        with torch.no_grad():
            want, mwant = net.forward_pre(i["x"], i["t"], i["context"], mt, gt)
            big = torch.full((B + 2, Cc, S, S), float("nan"), device=dev)
            mbig = torch.full((B + 2, K, S, S), float("nan"), device=dev)
            got, mgot = net.forward_pre(i["x"], i["t"], i["context"], mt, gt, out=big[1:B + 1], mask_out=mbig[1:B + 1])
        assert got.data_ptr() == big[1:].data_ptr()
        assert torch.isnan(big[0]).all() and torch.isnan(big[B + 1]).all()
        assert torch.isnan(mbig[0]).all() and torch.isnan(mbig[B + 1]).all()
        assert torch.isfinite(big[1:B + 1]).all() and torch.equal(big[1:B + 1], want)
        if mt is not None and not gt:
            assert mgot.data_ptr() == mbig[1:].data_ptr()
            assert torch.isfinite(mbig[1:B + 1]).all() and torch.equal(mbig[1:B + 1], mwant)
        else:   # no mask output in these modes: untouched
            assert mgot is None and mwant is None and torch.isnan(mbig).all()


@pytest.mark.parametrize("name", J.TINY)
def test_plain_path_reads_only_the_first_lx_pos_embed_rows(jg, dev, name):
    """Without a mask token a joint net gives the same bits whether pos_embed rows Lx .. Lm hold values or NaN."""
    kw, sd = J.state_dict(jg, name)
    i = _cuda(J.forward_inputs(jg, name), dev)
    Lx = 1 + kw["num_clip_token"] + (kw["img_size"] // kw["patch_size"]) ** 2
    outs = []
    for poison in (False, True):
        sd2 = dict(sd)
        if poison:
            sd2["pos_embed"] = sd["pos_embed"].clone()
            sd2["pos_embed"][:, Lx:] = float("nan")
        n = get_nnet(name="uvit_t2i", **kw)
        n.load_state_dict(sd2)
        n = n.to(dev).eval()
        with torch.no_grad():
            outs.append(n(i["x"], i["t"], i["context"]))
    assert torch.isfinite(outs[1]).all()
    assert torch.equal(outs[0], outs[1])


def test_persistent_gemm_rows_vs_oracle(dev):
    """B = 8 at Lm = 590: M = 4,720 >= 4,096 rows, where the block Linears take the persistent kernel (smaller
    batches of the other cases stay on the 128-tile kernel)."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    kw = dict(img_size=32, in_chans=4, patch_size=2, embed_dim=512, depth=2, num_heads=8, mlp_ratio=4, qkv_bias=False,
              mlp_time_embed=False, clip_dim=768, num_clip_token=77)
    sd = W.nnet_state_dict(dict(kw, name="uvit_t2i"), seed=11, init="random")
    net = get_nnet(name="uvit_t2i", **kw)
    net.load_state_dict(sd)
    net = net.to(dev).eval()
    g = torch.Generator().manual_seed(9)
    x = torch.randn(8, 4, 32, 32, generator=g)
    t = torch.rand(8, generator=g) * 998 + 1
    ctx = torch.randn(8, 77, 768, generator=g)
    mt = torch.randn(8, 8, 32, 32, generator=g)
    with torch.no_grad():
        eps, pm = net(x.to(dev), t.to(dev), ctx.to(dev), mask_token=mt.to(dev))
        ref_eps, ref_pm = uvit_ref.uvit_t2i_forward(sd, kw, x, t, ctx, mask_token=mt)
    errs = (rel(eps, ref_eps), rel(pm, ref_pm))
    print("persistent rows", errs)
    assert errs[0] < 2e-2 and errs[1] < 2e-2, errs


@pytest.mark.parametrize("name", J.FULL)
def test_full_size_forward_vs_reference(jg, dev, name):
    """mscoco_uvit_small_512_joint runs at L = 2126: the streamed attention family and the 64^2 head / unpatchify."""
    net = _net(jg, name, dev)
    i = _cuda(J.forward_inputs(jg, name), dev)
    with torch.no_grad():
        eps, pm = net(i["x"], i["t"], i["context"], mask_token=i["mask_token"])
    errs = (rel(eps, jg[f"{name}/eps_mask"]), rel(pm, jg[f"{name}/pred_mask"]))
    print(name, errs)
    assert errs[0] < 2e-2 and errs[1] < 2e-2, errs


def _sample_vs_reference(jg, dev, name, graph):
    net = _net(jg, name, dev)
    i = _cuda(J.sample_inputs(jg, name), dev)
    s = T2ISampler(net, cfg_scale=C.get_config(name)["cfg_scale"], steps=50, use_graph=graph)
    z, pm = s.sample(i["x"], i["context"], i["empty"], i["mask_token"])
    errs = (rel(z, jg[f"sample/{name}/z"]), rel(pm, jg[f"sample/{name}/pred_mask"]))
    print(name, "graph" if graph else "eager", errs)
    assert errs[0] < 1e-2 and errs[1] < 2e-2, errs


def test_full_size_sampler_vs_reference(jg, dev):
    _sample_vs_reference(jg, dev, "mscoco_uvit_small_joint", True)


@pytest.mark.parametrize("graph", [False, True])
def test_tiny_sampler_vs_reference(jg, dev, graph):
    _sample_vs_reference(jg, dev, "tiny_t2i_joint", graph)


def test_full_size_sampler_properties(jg, dev):
    """As test_gpu_configs.test_full_t2i_sampler_properties for the separate net: graph == eager, replay == replay,
    batch and lane invariance; a graph captured for other weights is dropped."""
    name = "mscoco_uvit_small_joint"
    net = _net(jg, name, dev)
    g = torch.Generator().manual_seed(7)
    z = torch.randn(3, 4, 32, 32, generator=g).to(dev)
    ctx = torch.randn(3, 77, 768, generator=g).to(dev)
    empty = torch.randn(77, 768, generator=g).to(dev)
    mt = torch.randn(3, 8, 32, 32, generator=g).to(dev)
    scale = C.get_config(name)["cfg_scale"]
    sg = T2ISampler(net, cfg_scale=scale, steps=50, use_graph=True)
    se = T2ISampler(net, cfg_scale=scale, steps=50, use_graph=False)
    a, pa = sg.sample(z, ctx, empty, mt)
    a, pa = a.clone(), pa.clone()
    b, pb = se.sample(z, ctx, empty, mt)
    assert torch.isfinite(a).all() and torch.isfinite(pa).all()
    assert torch.equal(a, b) and torch.equal(pa, pb)
    a2, pa2 = sg.sample(z, ctx, empty, mt)   # a second replay of the captured graph
    assert torch.equal(a, a2) and torch.equal(pa, pa2)
    c, pc = se.sample(z[:1], ctx[:1], empty, mt[:1])
    assert rel(c, a[:1]) < 1e-6 and rel(pc, pa[:1]) < 1e-6
    s2 = T2ISampler(net, cfg_scale=scale, steps=50, use_graph=True, lanes=2)
    d, pd = s2.sample(z, ctx, empty, mt)
    assert rel(d, a) < 1e-6 and rel(pd, pa) < 1e-6
    # other weights: the handle is rebuilt, so the graph holding the old device addresses must not be replayed
    kw, sd = J.state_dict(jg, name)
    try:
        net.load_state_dict(W.nnet_state_dict(dict(kw, name="uvit_t2i"), seed=12, init="random"))
        e, pe = sg.sample(z, ctx, empty, mt)
        f, pf = se.sample(z, ctx, empty, mt)
        assert torch.equal(e, f) and torch.equal(pe, pf)
        assert not torch.equal(e, a)
    finally:
        net.load_state_dict(sd)
