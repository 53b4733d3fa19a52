"""ORACLE (test infrastructure): fp32 CPU restatement of the LSimple training step.

Follows train_ldm_discrete.py:54-90 (Schedule, LSimple), 159-175 (train_step), train_t2i_discrete.py:111-142,148-224,
446-473 (the panoptic Schedule.sample, LSimple's mask branch, loss_eps.mean() + loss_mask.mean()), utils.py:475-488
(int2bits), sde.py:64-69,270-279 (VPSDE sample,
LSimple with ScoreModel.noise_pred: the net sees t * 999), utils.py:308-345 (torch.optim.AdamW, the 'customized'
warm-up LambdaLR, ema).  Gradients are torch autograd through oracle/uvit_ref.uvit_forward (itself pinned to the
reference's UViT at full size); the whole step is pinned to the reference's own training loop by
tests/golden/train_golden.npz (tests/golden/make_train_golden.py imports the reference).  Only tests/ use this.
"""
import numpy as np
import torch

from . import uvit_ref


def mos(a):
    """mean of squares per sample (train_ldm_discrete.py:49-50)."""
    return a.pow(2).flatten(1).mean(-1)


def lsimple_grads(sd, cfg, xt, t_in, y, target):
    """Per-sample loss mos(target - nnet(xt, t_in, y)) and d loss.mean() / d params (every key; zeros where a
    parameter does not reach the loss, e.g. unused label rows)."""
    params = {k: v.detach().clone().float().requires_grad_(True) for k, v in sd.items()}
    pred = uvit_ref.uvit_forward(params, cfg, xt, t_in, y)
    loss = mos(target - pred)
    loss.mean().backward()
    grads = {k: (p.grad if p.grad is not None else torch.zeros_like(p)).detach() for k, p in params.items()}
    return loss.detach(), grads


def adamw_step(p, g, m, v, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
    """torch.optim.AdamW single-tensor update (decoupled decay, bias-corrected moments); returns (p, m, v)."""
    b1, b2 = betas
    p = p * (1 - lr * weight_decay)
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    bc1 = 1 - b1 ** step
    bc2 = 1 - b2 ** step
    denom = v.sqrt() / (bc2 ** 0.5) + eps
    p = p - (lr / bc1) * m / denom
    return p, m, v


def customized_lr(base_lr, step, warmup_steps):
    """utils.customized_lr_scheduler: factor min(step / warmup, 1) (1 without warm-up) at scheduler step `step`."""
    return base_lr * (min(step / warmup_steps, 1) if warmup_steps > 0 else 1)


def ema(e, p, rate):
    """utils.ema: e <- rate e + (1 - rate) p."""
    return rate * e + (1 - rate) * p


def sd_betas():
    return (torch.linspace(0.00085 ** 0.5, 0.0120 ** 0.5, 1000, dtype=torch.float64) ** 2).numpy()


def discrete_sample(x0, np_seed, torch_seed):
    """Schedule.sample (train_ldm_discrete.py:75-80) under np.random.seed / torch.manual_seed: (n, eps, xn)."""
    betas = np.append(0., sd_betas())
    cum = (1. - betas).cumprod()
    np.random.seed(np_seed)
    torch.manual_seed(torch_seed)
    n = np.random.choice(list(range(1, 1001)), (len(x0),))
    eps = torch.randn_like(x0)
    a = torch.from_numpy(cum[n] ** 0.5).float().view(-1, 1, 1, 1)
    s = torch.from_numpy((1. - cum[n]) ** 0.5).float().view(-1, 1, 1, 1)
    return torch.tensor(n), eps, a * x0 + s * eps


def sde_sample(x0, torch_seed, beta_min=0.1, beta_max=20.0):
    """VPSDE sample (sde.py:64-69,72-113) under torch.manual_seed: (t, eps, xt)."""
    torch.manual_seed(torch_seed)
    t = torch.rand(x0.shape[0])
    integ = beta_min * t + (beta_max - beta_min) * t ** 2 * 0.5
    alpha = torch.exp(-integ)
    mean = alpha.sqrt().view(-1, 1, 1, 1) * x0
    std = (1. - alpha).sqrt()
    eps = torch.randn_like(x0)
    return t, eps, mean + std.view(-1, 1, 1, 1) * eps


def train_steps(sd, cfg, x0, y, draws, objective, opt, warmup_steps, ema_rate):
    """`len(draws)` reference training iterations on one batch: draws[i] = seeds of iteration i.  Returns (losses per
    iteration, the first iteration's grads, final params, final ema)."""
    p = {k: v.detach().clone().float() for k, v in sd.items()}
    m = {k: torch.zeros_like(v) for k, v in p.items()}
    v2 = {k: torch.zeros_like(v) for k, v in p.items()}
    e = {k: v.clone() for k, v in p.items()}
    losses, g0 = [], None
    for i, seeds in enumerate(draws):
        if objective == "discrete":
            n, eps, xt = discrete_sample(x0, *seeds)
            t_in = n.float()
        else:
            t, eps, xt = sde_sample(x0, seeds[1])
            t_in = t * 999
        loss, g = lsimple_grads(p, cfg, xt, t_in, y, eps)
        losses.append(loss)
        if g0 is None:
            g0 = g
        lr = customized_lr(opt["lr"], i, warmup_steps)
        for k in p:
            p[k], m[k], v2[k] = adamw_step(p[k], g[k], m[k], v2[k], i + 1, lr, opt["betas"], opt.get("eps", 1e-8),
                                           opt["weight_decay"])
            e[k] = ema(e[k], p[k], ema_rate)
    return losses, g0, p, e


def int2bits(x, n=8):
    """utils.int2bits (utils.py:475-488): integer masks (b, 1, h, w) -> bits (b, n, h, w), channel 0 = the most
    significant bit (x >> (n-1)), channel n-1 = x mod 2."""
    x = x.to(torch.int64)
    y = torch.cat([torch.bitwise_right_shift(x, i) for i in range(n - 1, -1, -1)], dim=1)
    return torch.remainder(y, 2).float()


def t2i_sample(x0, scaled, np_seed, torch_seed):
    """The t2i Schedule.sample with a panoptic mask (train_t2i_discrete.py:111-142) under np.random.seed /
    torch.manual_seed: n ~ U{1..1000}, eps = randn_like(x0), xn; eps_m = 2 randn_like(scaled), mask_n."""
    betas = np.append(0., sd_betas())
    cum = (1. - betas).cumprod()
    np.random.seed(np_seed)
    torch.manual_seed(torch_seed)
    n = np.random.choice(list(range(1, 1001)), (len(x0),))
    eps = torch.randn_like(x0)
    a = torch.from_numpy(cum[n] ** 0.5).float().view(-1, 1, 1, 1)
    s = torch.from_numpy((1. - cum[n]) ** 0.5).float().view(-1, 1, 1, 1)
    xn = a * x0 + s * eps
    eps_m = 2.0 * torch.randn_like(scaled)
    mask_n = a * scaled + s * eps_m
    return torch.tensor(n), eps, xn, eps_m, mask_n


def lsimple_t2i_grads(sd, cfg, xt, t_in, context, mask_n, eps, scaled):
    """Per-sample loss_eps = mos(eps - eps_pred), loss_mask = mos(mask_pred - scaled) of the separate-stream panoptic
    net (mask_token = mask_n) and d(loss_eps.mean() + loss_mask.mean()) / d params.  Returns (loss_eps, loss_mask,
    grads, used): grads are zeros for parameters the forward never touches, `used` the keys that got a gradient
    (torch.optim skips the others)."""
    params = {k: v.detach().clone().float().requires_grad_(True) for k, v in sd.items()}
    noise, y = uvit_ref.uvit_t2i_forward(params, cfg, xt, t_in, context, mask_token=mask_n, enable_panoptic=True)
    le, lm = mos(eps - noise), mos(y - scaled)
    (le.mean() + lm.mean()).backward()
    used = {k for k, p in params.items() if p.grad is not None}
    grads = {k: (p.grad if p.grad is not None else torch.zeros_like(p)).detach() for k, p in params.items()}
    return le.detach(), lm.detach(), grads, used



# ---- float64 references of the training step's kernels, one operation each (tests/test_gpu_train_kernels.py) -----
# Written from the reference's Python (libs/uvit.py, libs/uvit_t2i.py, sde.py, libs/timm.py), not from the kernels;
# tests/test_train_kernel_refs.py pins each to torch's own op.  Inputs of any dtype are taken to float64.

def gather_index(rows, rpg=0, gs=0, off=0):
    """Physical row of logical row r under a row gather: (r // rpg) * gs + off + r % rpg (rpg 0: r)."""
    r = torch.arange(rows)
    return r if rpg <= 0 else (r // rpg) * gs + off + r % rpg


def patchify_ref(imgs, p):
    """libs/uvit.py patchify: 'B C (h p1) (w p2) -> B (h w) (p1 p2 C)'."""
    B, C, H, W = imgs.shape
    return imgs.reshape(B, C, H // p, p, W // p, p).permute(0, 2, 4, 3, 5, 1).reshape(B, (H // p) * (W // p), p * p * C)


def unpatchify_ref(x, C, h, w):
    """libs/uvit.py unpatchify, 'B (h w) (p1 p2 C) -> B C (h p1) (w p2)', for an h x w grid of patches."""
    B, N, P = x.shape
    p = int(round((P // C) ** 0.5))
    assert h * w == N and p * p * C == P
    return x.reshape(B, h, w, p, p, C).permute(0, 5, 1, 3, 2, 4).reshape(B, C, h * p, w * p)


def patch_vectors_ref(imgs, p):
    """The operand of PatchEmbed's Conv2d(k = s = p) as a matmul: [B, (h w), (C p1 p2)], the conv weight's flatten."""
    B, C, H, W = imgs.shape
    return imgs.reshape(B, C, H // p, p, W // p, p).permute(0, 2, 4, 1, 3, 5).reshape(B, (H // p) * (W // p), C * p * p)


def patch_embed_ref(imgs, weight, bias, p):
    """PatchEmbed.forward (libs/uvit.py:129-135) with weight flattened to [D, C p p]: [B, N, D] float64."""
    return patch_vectors_ref(imgs.double(), p) @ weight.double().t() + bias.double()


def timestep_embedding_ref(t, dim, max_period=10000):
    """libs/uvit.py timestep_embedding in float64."""
    import math
    half = dim // 2
    freqs = torch.exp(-math.log(max_period) * torch.arange(half, dtype=torch.float64) / half)
    args = t.double()[:, None] * freqs[None]
    emb = torch.cat([torch.cos(args), torch.sin(args)], dim=-1)
    if dim % 2:
        emb = torch.cat([emb, torch.zeros_like(emb[:, :1])], dim=-1)
    return emb, args


def assemble_ref(imgs, p, patch_w, patch_b, pos, t=None, time_emb=None, y=None, label_emb=None, ctx_tokens=None,
                 label_first=True):
    """Token assembly: libs/uvit.py:201-212 ([label?][time][patches] + pos_embed), libs/uvit_t2i.py:401-409
    ([time][context][patches] + pos_embed); without t / time_emb the patch rows alone (the t2i mask stream).
    Returns [B, L, D] float64 for the L rows present."""
    x = patch_embed_ref(imgs, patch_w, patch_b, p)
    D = x.shape[-1]
    if ctx_tokens is not None:
        x = torch.cat((ctx_tokens.double(), x), dim=1)
    if t is not None or time_emb is not None:
        tok = time_emb.double() if time_emb is not None else timestep_embedding_ref(t, D)[0]
        x = torch.cat((tok[:, None], x), dim=1)
    if y is not None:
        x = torch.cat((label_emb.double()[y][:, None], x), dim=1)
    return x + pos.double()[: x.shape[1]]


def gelu_ref(u):
    """nn.GELU (libs/timm.py:102): u Phi(u), Phi by erfc so that the tail u << 0 keeps its digits."""
    u = u.double()
    return u * 0.5 * torch.special.erfc(-u * 0.7071067811865476)


def gelu_grad_ref(u):
    """d gelu / du = Phi(u) + u phi(u)."""
    u = u.double()
    return 0.5 * torch.special.erfc(-u * 0.7071067811865476) + u * torch.exp(-0.5 * u * u) * 0.3989422804014327


def lsimple_ref(pred, target, gscale, tanh_bwd=False):
    """sde.py LSimple / mos: loss[b] = mean (target - pred)^2 and d(gscale * sum_b loss[b]) / d pred; with tanh_bwd
    pred = tanh(u) was applied by the caller and the gradient is w.r.t. u (libs/uvit_t2i.py:513).
    Returns (loss, dpred, terms) with terms = (target - pred)^2, the loss's summands."""
    y = pred.double().flatten(1)
    d = target.double().flatten(1) - y
    per = y.shape[1]
    loss = (d * d).mean(-1)
    g = -2.0 * gscale / per * d
    if tanh_bwd:
        g = g * (1.0 - y * y)
    return loss, g.reshape(pred.shape), d * d


def conv3x3_backward_ref(dout, x, w):
    """Gradients of nn.Conv2d(C, C, 3, padding=1) (libs/uvit.py:183 final_layer) by float64 autograd: (din, dw, db)."""
    x = x.double().requires_grad_(True)
    w = w.double().requires_grad_(True)
    b = torch.zeros(w.shape[0], dtype=torch.float64, requires_grad=True)
    out = torch.nn.functional.conv2d(x, w, b, padding=1)
    out.backward(dout.double())
    return x.grad, w.grad, b.grad


def head_ref(tok, weight, bias, C, h, w, act_tanh=False):
    """decoder_pred + unpatchify (libs/uvit.py:225-228) [+ tanh, libs/uvit_t2i.py:513]: tok [B, N, D] -> [B, C, H, W]."""
    out = unpatchify_ref(tok.double() @ weight.double().t() + bias.double(), C, h, w)
    return torch.tanh(out) if act_tanh else out


def head_backward_ref(dpre, weight, C, p):
    """Backward of head_ref without tanh by autograd: (dtok [B, N, P] = the gradient at decoder_pred's output,
    dx [B, N, D] = the gradient at its input)."""
    B, _, H, W = dpre.shape
    h, w = H // p, W // p
    P, D = weight.shape
    lin = torch.zeros(B, h * w, P, dtype=torch.float64, requires_grad=True)
    unpatchify_ref(lin, C, h, w).backward(dpre.double())
    x = torch.zeros(B, h * w, D, dtype=torch.float64, requires_grad=True)
    (x @ weight.double().t()).backward(lin.grad)
    return lin.grad, x.grad


def layernorm_ref(x, gamma, beta, eps=1e-5):
    return torch.nn.functional.layer_norm(x.double(), (x.shape[-1],), gamma.double(), beta.double(), eps)


def layernorm_backward_ref(x, dh, gamma, eps=1e-5):
    """(dx, dgamma, dbeta) of nn.LayerNorm over rows x [rows, D] with output gradient dh, float64 autograd."""
    x = x.double().requires_grad_(True)
    g = gamma.double().requires_grad_(True)
    b = torch.zeros_like(g).requires_grad_(True)
    torch.nn.functional.layer_norm(x, (x.shape[-1],), g, b, eps).backward(dh.double())
    return x.grad, g.grad, b.grad


def adamw_ema_ref(p, g, m, v, e, step, lr, betas, eps, weight_decay, ema_rate):
    """One torch.optim.AdamW step (utils.py:308-345) followed by utils.ema, in float64: (p, m, v, ema, update) with
    update = the Adam term subtracted from the decayed parameter."""
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    p0 = p * (1 - lr * weight_decay)
    p1, m1, v1 = adamw_step(p, g, m, v, step, lr, betas, eps, weight_decay)
    e1 = ema(e.double(), p1, ema_rate) if e is not None else None
    return p1, m1, v1, e1, p0 - p1
