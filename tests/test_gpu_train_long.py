"""The training step past the head-in-LDS attention backward's limits (608 tokens per stream at head dim 64, 415 at
72): a 64 x 64 latent at patch 2, so the t2i streams have Lx = 1102 / Lm = 2126 tokens (the reference's 512^2
text-to-image config) and the class-conditional U-ViT L = 1026 (at head dim 72).  The attention backward of these
steps runs on the streaming kernels (tests/test_gpu_attn_bwd_stream.py checks them alone).

Bounds as in tests/test_gpu_train.py for tiny nets: losses rel-L2 <= 1e-2, each used gradient rel-L2 <= 3e-2 against
the oracle's fp32 autograd (oracle/train_ref.py); the forward bound 2e-2."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _state(name, lanes=1, seed=11):
    from panopticdiffusionmodels_amd import configs, weights
    from panopticdiffusionmodels_amd.train import HipTrainState
    full = configs.get_config(name)
    sd = weights.nnet_state_dict(full["nnet"], seed=seed, init="random")
    st = HipTrainState(full["nnet"], DEV, optimizer=full["optimizer"], lr_scheduler=dict(warmup_steps=-1), ema_rate=0.9,
                       lanes=lanes)
    st.load_state_dict(sd)
    kw = dict(full["nnet"])
    kw.pop("name")
    return full, kw, sd, st


def _t2i_inputs(B, S=64, nctx=77, clip=64, seed=8):
    from oracle import train_ref
    g = torch.Generator().manual_seed(seed)
    xt = torch.randn(B, 4, S, S, generator=g)
    t = torch.rand(B, generator=g) * 999
    ctx = torch.randn(B, nctx, clip, generator=g)
    scaled = train_ref.int2bits(torch.randint(0, 201, (B, 1, S, S), generator=g)) * 2 - 1
    mask_n = scaled * 0.5 + torch.randn(B, 8, S, S, generator=g)
    eps = torch.randn(B, 4, S, S, generator=g)
    return xt, t, ctx, mask_n, eps, scaled


def test_t2i_512_step_vs_oracle():
    """tiny_t2i_train_512 (Lx 1102, Lm 2126), 2 images: both losses, every used gradient, zeros for the unused."""
    from oracle import train_ref
    full, kw, sd, st = _state("tiny_t2i_train_512")
    xt, t, ctx, mask_n, eps, scaled = _t2i_inputs(2)
    loss, loss_m = st.forward_backward_t2i(xt, t, ctx, mask_n, eps, scaled)
    le, lm, gref, used = train_ref.lsimple_t2i_grads(sd, kw, xt, t, ctx, mask_n, eps, scaled)
    print("losses", rel(loss, le), rel(loss_m, lm))
    assert rel(loss, le) < 1e-2 and rel(loss_m, lm) < 1e-2
    grads = st.grads()
    bad = {k: rel(grads[k], gref[k]) for k in used if float(gref[k].norm()) > 0}
    print("worst gradients", sorted(bad.items(), key=lambda kv: -kv[1])[:3])
    assert max(bad.values()) < 3e-2, sorted(bad.items(), key=lambda kv: -kv[1])[:5]
    assert len(used) < len(grads)
    for k in set(grads) - used:
        assert float(grads[k].abs().max()) == 0.0, k


def test_h72_long_step_vs_oracle():
    """tiny_uvit_train_h_long (8 heads x 72, L = 1026), 2 images: loss and every gradient."""
    from oracle import train_ref
    full, kw, sd, st = _state("tiny_uvit_train_h_long")
    g = torch.Generator().manual_seed(9)
    B = 2
    xt = torch.randn(B, 4, 64, 64, generator=g)
    t = torch.rand(B, generator=g) * 999
    y = torch.tensor([3, 10])
    eps = torch.randn(B, 4, 64, 64, generator=g)
    loss = st.forward_backward(xt, t, y, eps)
    lref, gref = train_ref.lsimple_grads(sd, kw, xt, t, y, eps)
    print("loss", rel(loss, lref))
    assert rel(loss, lref) < 1e-2
    grads = st.grads()
    bad = {k: rel(grads[k], gref[k]) for k in grads if float(gref[k].norm()) > 0}
    print("worst gradients", sorted(bad.items(), key=lambda kv: -kv[1])[:3])
    assert max(bad.values()) < 3e-2, sorted(bad.items(), key=lambda kv: -kv[1])[:5]


def test_t2i_512_train_step_moves_parameters():
    """One whole train_step (noise draw, step, AdamW + EMA) on tiny_t2i_train_512: finite everywhere, parameters
    moved."""
    import numpy as np
    full, kw, sd, st = _state("tiny_t2i_train_512")
    g = torch.Generator().manual_seed(5)
    x0 = torch.randn(2, 4, 64, 64, generator=g).to(DEV)
    ctx = torch.randn(2, 77, 64, generator=g).to(DEV)
    pan = torch.randint(0, 201, (2, 1, 64, 64), generator=g)
    out = st.train_step(x0, context=ctx, panoptic=pan, rng=np.random.RandomState(0))
    assert bool(torch.isfinite(out["loss"])) and bool(torch.isfinite(out["loss_mask"]))
    p = st.state_dict()
    moved = 0
    for k, v in p.items():
        assert bool(torch.isfinite(v).all()), k
        moved += int(not torch.equal(v.cpu(), sd[k].float()))
    for k, v in st.ema_state_dict().items():
        assert bool(torch.isfinite(v).all()), k
    assert moved > len(p) // 2, moved


def test_t2i_512_lanes_equal_single():
    """Two concurrent half-batch lanes give the single-lane losses and gradients on tiny_t2i_train_512 (each lane has
    its own workspace and so its own attention-backward scratch)."""
    xt, t, ctx, mask_n, eps, scaled = _t2i_inputs(3, seed=4)
    outs, grads, used = [], [], None
    for lanes in (1, 2):
        full, kw, sd, st = _state("tiny_t2i_train_512", lanes=lanes)
        outs.append(tuple(v.cpu() for v in st.forward_backward_t2i(xt, t, ctx, mask_n, eps, scaled)))
        grads.append({k: v.cpu() for k, v in st.grads().items()})
        used = set(st.index) - st.stateless_params()
        del st
    for a, b in zip(outs[0], outs[1]):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-7)
    g1, g2 = grads
    for k in g1:
        if k in used:
            assert rel(g2[k], g1[k]) < 1e-4 or float(g1[k].norm()) == 0, k
        else:
            assert float(g2[k].abs().max()) == 0.0, k


def test_t2i_forward_64x64_latent_vs_oracle():
    """Sampling at these lengths: one forward of a tiny_t2i-width net with img_size 64 and a mask token (image stream
    1 + 5 + 1024 tokens, mask stream 2054: the key-streaming forward attention) through HipNet."""
    from oracle import uvit_ref
    from panopticdiffusionmodels_amd import configs, weights
    from panopticdiffusionmodels_amd.utils import get_nnet
    cfg = configs.nnet_kwargs("tiny_t2i")
    cfg["img_size"] = 64
    sd = weights.nnet_state_dict(cfg, seed=11, init="random")
    net = get_nnet(**cfg)
    net.load_state_dict(sd)
    net = net.cuda().eval()
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 4, 64, 64, generator=g)
    t = torch.rand(2, generator=g) * 999
    ctx = torch.randn(2, cfg["num_clip_token"], cfg["clip_dim"], generator=g)
    mt = torch.randn(2, 8, 64, 64, generator=g)
    eps, pm = net(x.cuda(), t.cuda(), ctx.cuda(), mask_token=mt.cuda())
    kw = dict(cfg)
    kw.pop("name")
    with torch.no_grad():
        eref, pref = uvit_ref.uvit_t2i_forward({k: v.float() for k, v in sd.items()}, kw, x, t, ctx, mask_token=mt,
                                               enable_panoptic=True)
    print("forward", rel(eps, eref), rel(pm, pref))
    assert rel(eps, eref) <= 2e-2 and rel(pm, pref) <= 2e-2
