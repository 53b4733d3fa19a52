"""The float64 references of tests/test_gpu_train_kernels.py (oracle/train_ref.py) pinned to torch's own ops, without
a GPU: a reference that shared a kernel's mistake (a column order, a derivative, a bias correction) fails here.  Also
the argument checks of the kernel entry points, which return PDM_ERR_ARG before any launch and so run without a GPU.
"""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

from oracle import train_ref as R

TIGHT = 1e-12


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _close(a, b, tol=TIGHT):
    d = float((a.detach().double() - b.detach().double()).abs().max())
    s = float(b.detach().double().abs().max())
    assert d <= tol * max(s, 1.0), (d, s)


@pytest.mark.parametrize("C,p,H,W", [(3, 2, 6, 10), (4, 4, 8, 12), (5, 3, 6, 9), (8, 2, 4, 6)])
def test_patch_orders_vs_conv2d_and_unfold(C, p, H, W):
    g = _gen(C * 100 + p)
    img = torch.randn(2, C, H, W, generator=g, dtype=torch.float64)
    D = 7
    conv = torch.nn.Conv2d(C, D, kernel_size=p, stride=p).double()
    with torch.no_grad():
        conv.weight.copy_(torch.randn(D, C, p, p, generator=g, dtype=torch.float64))
        conv.bias.copy_(torch.randn(D, generator=g, dtype=torch.float64))
        want = conv(img).flatten(2).transpose(1, 2)           # PatchEmbed.forward
    _close(R.patch_embed_ref(img, conv.weight.reshape(D, -1), conv.bias, p), want)
    # the operand's (c, p1, p2) columns are torch's unfold; the reference patchify's (p1, p2, c) a permutation of them
    pv = F.unfold(img, kernel_size=p, stride=p).transpose(1, 2)
    assert torch.equal(R.patch_vectors_ref(img, p), pv)
    N = pv.shape[1]
    assert torch.equal(R.patchify_ref(img, p), pv.reshape(2, N, C, p, p).permute(0, 1, 3, 4, 2).reshape(2, N, -1))


@pytest.mark.parametrize("C,p,h,w", [(3, 2, 3, 5), (4, 4, 2, 3), (5, 3, 2, 2)])
def test_unpatchify_vs_its_definition(C, p, h, w):
    """'B (h w) (p1 p2 C) -> B C (h p1) (w p2)' element by element, and as the inverse of patchify."""
    x = torch.randn(2, h * w, p * p * C, generator=_gen(p), dtype=torch.float64)
    out = R.unpatchify_ref(x, C, h, w)
    assert out.shape == (2, C, h * p, w * p)
    for i in range(h):
        for j in range(w):
            for p1 in range(p):
                for p2 in range(p):
                    for c in range(C):
                        assert torch.equal(out[:, c, i * p + p1, j * p + p2], x[:, i * w + j, (p1 * p + p2) * C + c])
    assert torch.equal(R.patchify_ref(out, p), x)
    # the square case is the reference's own signature: h = w = sqrt(N)
    if h == w:
        fold = F.fold(x.reshape(2, h * w, p, p, C).permute(0, 4, 2, 3, 1).reshape(2, C * p * p, h * w), (h * p, w * p),
                      kernel_size=p, stride=p)
        assert torch.equal(out, fold)


def test_gelu_and_derivative_vs_torch():
    u = torch.cat([torch.linspace(-12, 12, 4801, dtype=torch.float64), torch.tensor([-40.0, -1e-30, 0.0, 1e-30, 40.0],
                                                                                   dtype=torch.float64)])
    u = u.requires_grad_(True)
    y = F.gelu(u)
    y.sum().backward()
    ref, dref = R.gelu_ref(u.detach()), R.gelu_grad_ref(u.detach())
    # F.gelu evaluates 1 + erf: absolute error ~1e-16 |u| in the negative tail, where erfc keeps relative accuracy
    assert float((ref - y.detach()).abs().max()) <= 4e-15
    assert float((dref - u.grad).abs().max()) <= 4e-15
    # the tail by its asymptote: gelu(u) -> -phi(u) (1 - 1/u^2), u -> -inf
    t = torch.tensor([-8.0, -10.0, -12.0], dtype=torch.float64)
    asym = -torch.exp(-0.5 * t * t) * 0.3989422804014327 * (1 - 1 / t ** 2 + 3 / t ** 4)
    assert float(((R.gelu_ref(t) - asym) / asym).abs().max()) < 5e-3


@pytest.mark.parametrize("wd,with_g2", [(0.0, False), (0.03, True)])
def test_adamw_ema_vs_torch_optim_three_steps(wd, with_g2):
    g = _gen(3)
    n, lr, betas, eps, rate = 257, 2e-3, (0.9, 0.99), 1e-8, 0.99
    p0 = torch.randn(n, generator=g, dtype=torch.float64)
    prm = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([prm], lr=lr, betas=betas, eps=eps, weight_decay=wd)
    p, m, v, e = p0.clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64), p0.clone()
    e_t = p0.clone()
    for step in (1, 2, 3):
        gr = torch.randn(n, generator=g, dtype=torch.float64) * 10.0 ** (step - 2)
        if with_g2:
            gr = gr + torch.randn(n, generator=g, dtype=torch.float64)
        prm.grad = gr.clone()
        opt.step()
        e_t = rate * e_t + (1 - rate) * prm.detach()          # utils.ema
        p_prev = p
        p, m, v, e, upd = R.adamw_ema_ref(p, gr, m, v, e, step, lr, betas, eps, wd, rate)
        _close(p, prm.detach())
        _close(e, e_t)
        st = opt.state[prm]
        _close(m, st["exp_avg"])
        _close(v, st["exp_avg_sq"])
        _close(upd, p_prev * (1 - lr * wd) - p)               # the Adam term subtracted from the decayed parameter
    assert R.adamw_ema_ref(p, gr, m, v, None, 4, lr, betas, eps, wd, rate)[3] is None


@pytest.mark.parametrize("tanh_bwd", [False, True])
def test_lsimple_vs_autograd(tanh_bwd):
    g = _gen(9)
    B, shape, gscale = 3, (2, 5, 7), 0.37
    u = (torch.randn(B, *shape, generator=g, dtype=torch.float64) * 3).requires_grad_(True)
    tgt = torch.randn(B, *shape, generator=g, dtype=torch.float64)
    pred = torch.tanh(u) if tanh_bwd else u
    loss = (tgt - pred).pow(2).flatten(1).mean(-1)              # mos(noise - noise_pred)
    (gscale * loss.sum()).backward()
    l, d, terms = R.lsimple_ref(pred.detach(), tgt, gscale, tanh_bwd)
    _close(l, loss.detach())
    _close(d, u.grad)
    _close(terms.mean(-1), loss.detach())


@pytest.mark.parametrize("C,p,H,W,tanh", [(3, 2, 6, 6, False), (4, 4, 8, 12, False), (8, 2, 8, 12, True)])
def test_head_refs_vs_autograd(C, p, H, W, tanh):
    g = _gen(C)
    B, D, h, w = 2, 16, H // p, W // p
    lin = torch.nn.Linear(D, p * p * C).double()
    tok = torch.randn(B, h * w, D, generator=g, dtype=torch.float64, requires_grad=True)
    out = R.unpatchify_ref(lin(tok), C, h, w)                   # decoder_pred, unpatchify
    if tanh:
        out = torch.tanh(out)
    _close(R.head_ref(tok.detach(), lin.weight.detach(), lin.bias.detach(), C, h, w, tanh), out.detach())
    if not tanh:
        dpre = torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
        out.backward(dpre)
        dtok, dx = R.head_backward_ref(dpre, lin.weight.detach(), C, p)
        _close(dx, tok.grad)
        assert torch.equal(dtok, R.patchify_ref(dpre, p))       # the gathered gradient


def test_timestep_embedding_and_assembly_vs_module_code():
    from panopticdiffusionmodels_amd.libs.uvit import timestep_embedding
    t = torch.tensor([0.0, 0.5, 999.0])
    for D in (64, 260, 7):
        emb, args = R.timestep_embedding_ref(t, D)
        want = timestep_embedding(t, D).double()
        bound = 2.0 ** -22 + args.abs() * 2.0 ** -21
        bound = torch.cat([bound, bound, torch.zeros(3, D % 2, dtype=torch.float64)], -1)
        assert bool(((emb - want).abs() <= bound).all())
    g = _gen(1)
    B, C, p, H, D, ncls = 2, 3, 2, 4, 8, 5
    img = torch.randn(B, C, H, H, generator=g, dtype=torch.float64)
    w, b = torch.randn(D, C * p * p, generator=g, dtype=torch.float64), torch.randn(D, generator=g, dtype=torch.float64)
    lab = torch.randn(ncls, D, generator=g, dtype=torch.float64)
    y = torch.tensor([4, 0])
    pos = torch.randn(6, D, generator=g, dtype=torch.float64)
    x = R.patch_embed_ref(img, w, b, p)
    tt = R.timestep_embedding_ref(t[:2], D)[0]
    want = torch.cat((lab[y][:, None], tt[:, None], x), 1) + pos           # libs/uvit.py:201-212
    assert torch.equal(R.assemble_ref(img, p, w, b, pos, t=t[:2], y=y, label_emb=lab), want)
    ctx = torch.randn(B, 1, D, generator=g, dtype=torch.float64)
    te = torch.randn(B, D, generator=g, dtype=torch.float64)
    want = torch.cat((te[:, None], ctx, x), 1) + pos                       # libs/uvit_t2i.py:401-409
    assert torch.equal(R.assemble_ref(img, p, w, b, pos, time_emb=te, ctx_tokens=ctx), want)
    assert torch.equal(R.assemble_ref(img, p, w, b, pos), x + pos[:4])


def test_conv_and_layernorm_refs_are_torch_autograd():
    g = _gen(4)
    x = torch.randn(2, 3, 5, 4, generator=g)
    w = torch.randn(3, 3, 3, 3, generator=g)
    dout = torch.randn(2, 3, 5, 4, generator=g)
    din, dw, db = R.conv3x3_backward_ref(dout, x, w)
    _close(din, F.conv_transpose2d(dout.double(), w.double(), padding=1))
    _close(db, dout.double().sum((0, 2, 3)))
    _close(dw, torch.nn.grad.conv2d_weight(x.double(), w.shape, dout.double(), padding=1))
    xr, dh, gm = torch.randn(7, 12, generator=g), torch.randn(7, 12, generator=g), torch.rand(12, generator=g) + 0.5
    dx, dg, dbt = R.layernorm_backward_ref(xr, dh, gm)
    xh = (xr.double() - xr.double().mean(-1, keepdim=True)) / torch.sqrt(xr.double().var(-1, unbiased=False,
                                                                                        keepdim=True) + 1e-5)
    _close(dg, (dh.double() * xh).sum(0))
    _close(dbt, dh.double().sum(0))
    assert list(R.gather_index(6, 3, 5, 2)) == [2, 3, 4, 7, 8, 9] and list(R.gather_index(3)) == [0, 1, 2]


# ---- the entry points' argument checks: PDM_ERR_ARG before any launch, so no GPU is needed ----------------------

@pytest.fixture(scope="module")
def lib():
    from panopticdiffusionmodels_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libpdm.so not built")
    return _lib.load()


def test_entries_reject_bad_arguments_before_launching(lib):
    from panopticdiffusionmodels_amd import _lib
    P = ctypes.c_void_p
    a = 4096                       # an aligned, never dereferenced address: every call below must fail its checks
    ARG = 1
    big = 1 << 20
    # dW: N % 4 != 0 with a bias; misaligned bias
    assert lib.pdm_wgrad_gather(P(a), 8, 0, 0, 0, P(a), 8, 0, 0, 0, P(a), 8, 32, 6, 8, 0, P(a), 0, None, 0, None) == ARG
    assert lib.pdm_wgrad_gather(P(a), 8, 0, 0, 0, P(a), 8, 0, 0, 0, P(a), 8, 32, 8, 8, 0, P(a + 4), 0, None, 0,
                                None) == ARG
    # column sums: ncols % 4, odd scratch size
    assert lib.pdm_colsum(P(a), 0, 8, 4, 6, 0, 0, 0, P(a), 0, None, 0, None) == ARG
    assert lib.pdm_colsum(P(a), 0, 8, 4, 8, 0, 0, 0, P(a), 0, P(a), 40, None) == ARG
    # LayerNorm backward: D past 2048, D % 4, scratch below one block's share (39 D and 0 bytes), ldx < D
    def lnb(D, scratch_bytes, ldx=None):
        ldx = D if ldx is None else ldx
        return lib.pdm_layernorm_backward_rows(P(a), ldx, P(a), 0, D, P(a), P(a), ldx, None, P(a), P(a), 7, D, 0, 0, 0,
                                               1e-5, 0, 0, P(a), scratch_bytes, None)
    assert lnb(2052, big) == ARG and lnb(66, big) == ARG
    assert lnb(64, 40 * 64 - 32) == ARG and lnb(64, 0) == ARG and lnb(64, 7 * 64) == ARG
    assert b"40 D" in lib.pdm_last_error()
    assert lnb(64, big, ldx=60) == ARG
    assert lib.pdm_layernorm_rows(P(a), 2052, P(a), P(a), P(a), 2052, 4, 2052, 4, 0, 0, 1e-5, None) == ARG
    assert lib.pdm_layernorm_rows(P(a), 64, P(a), P(a), P(a), 64, 4, 64, 0, 0, 0, 1e-5, None) == ARG
    # GELU: n % 8
    assert lib.pdm_gelu_forward(P(a), P(a), 12, None) == ARG
    assert lib.pdm_gelu_backward(P(a), P(a), 12, None) == ARG
    assert lib.pdm_lsimple(P(a), P(a), P(a), P(a), 0, 5, 1.0, 0, None) == ARG
    assert lib.pdm_conv3x3_backward(P(a), P(a), P(a), P(a), P(a), P(a), 1, 0, 4, 4, None) == ARG
    # head: P = p p C > 64 both ways; D % 8; image not divisible
    assert lib.pdm_head_forward(P(a), 64, 9, 0, P(a), P(a), P(a), 1, 64, 5, 4, 12, 12, 80, 0, None) == ARG
    assert lib.pdm_head_forward(P(a), 68, 9, 0, P(a), P(a), P(a), 1, 68, 4, 2, 6, 6, 16, 0, None) == ARG
    assert lib.pdm_head_forward(P(a), 64, 9, 0, P(a), P(a), P(a), 1, 64, 4, 2, 7, 6, 16, 0, None) == ARG
    assert lib.pdm_head_backward(P(a), P(a), P(a), P(a), 1, 64, 5, 4, 12, 12, 80, None) == ARG
    assert lib.pdm_head_backward(P(a), P(a), P(a), P(a), 1, 64, 4, 2, 6, 6, 8, None) == ARG
    q = _lib.PdmAssembleArgs()
    q.img = q.patch_w = q.patch_b = q.pos = q.out = a
    q.C, q.Himg, q.Wimg, q.p, q.B, q.D, q.ld_out, q.L_total = 3, 4, 4, 2, 1, 64, 64, 4
    q.row0_patch, q.time_row, q.label_row, q.ctx_row = 1, -1, -1, -1           # 1 + 4 patches > 4 rows
    assert lib.pdm_assemble(ctypes.byref(q), None) == ARG
    q.row0_patch, q.time_row = 0, 0                                            # a time row without t / time_emb
    assert lib.pdm_assemble(ctypes.byref(q), None) == ARG
    assert lib.pdm_patchify(P(a), P(a), 1, 3, 4, 4, 2, 8, None) == ARG         # ldp < C p p
    assert lib.pdm_label_scatter(P(a), 5, 5, 64, P(a), P(a), 2, None) == ARG   # row outside the sequence
    assert lib.pdm_rows_add_cast(P(a), P(a), 0, 0, 0, P(a), 0, 0, 0, 4, 6, 0, None) == ARG
    assert lib.pdm_add_cast(P(a), None, P(a), 6, None) == ARG
    assert lib.pdm_transpose_bf16(P(a), P(a), 6, 8, None) == ARG
    assert lib.pdm_transpose_bf16(P(a), P(a), 8, 6, None) == ARG


# ---- the bounds of tests/test_gpu_train_kernels.py reject the bugs they are there for (emulated in float64) ------

def _worst(out, ref, bound):
    return float(((out - ref).abs() / bound).max())


def test_bounds_reject_the_bugs_they_are_for():
    g = _gen(21)
    u = 2.0 ** -24
    # AdamW at step 2 with step 1's second bias correction
    n, lr, b1, b2, eps = 4096, 2e-4, 0.9, 0.999, 1e-8
    p, gr, m = (torch.randn(n, generator=g, dtype=torch.float64) for _ in range(3))
    v = torch.rand(n, generator=g, dtype=torch.float64)
    rp, rm, rv, _, upd = R.adamw_ema_ref(p, gr, m * 0.3, v, None, 2, lr, (b1, b2), eps, 0.0, 0.99)
    bad = p - (lr / (1 - b1 ** 2)) * rm / (rv.sqrt() / (1 - b2 ** 1) ** 0.5 + eps)
    assert _worst(bad, rp, 2.0 ** -23 * rp.abs() + 2.0 ** -21 * upd.abs()) > 100
    # the fused bias gradient of a split dW without the tail chunk's last 32-row stage (M 1100 = 576 + 524)
    a = torch.randn(1100, 64, generator=g).bfloat16().double()
    bad = a[:1088].sum(0)
    assert _worst(bad, a.sum(0), (1100 + 2) * u * a.abs().sum(0)) > 10
    # a column sum whose second pass reads the other ping-pong half (stale partials of equal magnitude)
    x = torch.randn(257, 8, generator=g, dtype=torch.float64)
    bad = torch.randn(17, 8, generator=g, dtype=torch.float64).sum(0) * 4
    assert _worst(bad, x.sum(0), (257 + 2) * u * x.abs().sum(0)) > 100
    # (c, p1, p2) against (p1, p2, c): bit-different at every tested (C, p), p = 2 included
    for C, p in ((3, 2), (4, 4), (8, 2), (4, 2)):
        img = torch.randn(1, C, 2 * p, 3 * p, generator=g)
        assert not torch.equal(R.patch_vectors_ref(img, p), R.patchify_ref(img, p))
    # a GELU derivative that is off in the tail only: the tanh approximation's, at dg = 1
    uu = torch.linspace(-6, 6, 1201, dtype=torch.float64).requires_grad_(True)
    F.gelu(uu, approximate="tanh").sum().backward()
    ref = R.gelu_grad_ref(uu.detach())
    hu = torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126))) - 8)
    assert _worst(uu.grad, ref, hu + (1 + uu.detach().abs()) * 2.0 ** -23) > 2
