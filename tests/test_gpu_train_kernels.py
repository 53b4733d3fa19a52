"""The training step's kernels one by one (include/pdm.h pdm_wgrad_gather ... pdm_transpose_bf16, pdm_train_adamw): each
HIP kernel against float64 torch (oracle/train_ref.py, pinned to torch's own ops by tests/test_train_kernel_refs.py) on
the same rounded operands, at the smallest shapes that reach every index computation, tail and branch.

Error measure (u = 2^-24):
  * an fp32 reduction of n terms: every element within (n + 2) u R|.|, R|.| the same float64 reduction over the
    absolute values of the terms -- no summation order can exceed it; a prior value added (accumulate) is one more term;
  * a bf16 output: 0.5 bf16 ulp of the float64 value on top of that;
  * a copy, a cast, a single fp32 add, a permutation: bit-equal to torch;
  * the kernels that are not plain reductions carry their own bound, derived where it is used.
Every output buffer is pre-filled with a sentinel: what the kernel must not touch is checked bit-unchanged, padding it
must zero is checked zero.  Rows a gather skips and padding columns of inputs hold NaN, so a read of a wrong row or
column shows up.  Inputs come from a seeded CPU torch.Generator.

Every test records the worst fraction of its bound (printed; the MI355X figures are in DESIGN.md 5d).
"""
import pytest
import torch

from oracle import train_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
NAN = float("nan")
SENT = -12345.0
BF = torch.bfloat16
WORST = {}


@pytest.fixture(scope="module")
def lib():
    from panopticdiffusionmodels_amd import _lib
    _lib.load()
    yield _lib
    print("\nworst fraction of the bound per kernel:")
    for k in sorted(WORST):
        print(f"  {k}: {WORST[k]:.3f}")


@pytest.fixture(scope="module")
def scratch64():
    return torch.empty(16 << 20, dtype=torch.float32, device=DEV)   # 64 MiB


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a.cpu()), bits(b.cpu()))


def half_ulp_bf16(ref):
    e = torch.floor(torch.log2(ref.double().abs().clamp_min(2.0 ** -126)))
    return torch.exp2(e - 8)


def hold(kernel, out, ref, bound, what=""):
    """Every element of out within `bound` of ref (float64); NaN / inf count as infinite.  Records the worst fraction."""
    out, ref, bound = out.detach().cpu().double(), ref.detach().cpu().double(), bound.detach().cpu().double()
    assert out.shape == ref.shape == bound.shape, (kernel, what, out.shape, ref.shape, bound.shape)
    err = (out - ref).abs()
    frac = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0))
    frac = torch.nan_to_num(frac, nan=float("inf"), posinf=float("inf"))
    worst = float(frac.max()) if frac.numel() else 0.0
    WORST[kernel] = max(WORST.get(kernel, 0.0), worst)
    print(f"{kernel} {what}: worst |d| / bound = {worst:.3f}")
    assert worst <= 1.0, (kernel, what, worst, int((frac > 1).sum()))
    return worst


def rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def gathered(g, rows, cols, ld, gather, dtype, scale=1.0):
    """(physical [R, ld] tensor with NaN in skipped rows and padding columns, the logical [rows, cols] values)."""
    idx = R.gather_index(rows, *gather)
    phys = torch.full((int(idx.max()) + 1 + (2 if gather[0] else 0), ld), NAN)
    vals = (randn(g, rows, cols, scale=scale)).to(dtype)
    phys[idx, :cols] = vals.float()
    return phys.to(dtype), vals, idx


# ---------------------------------------------------------------------------------------------------------------
# dW with row gathers and the fused bias gradient

WGRAD_CASES = {
    # name: (M, N, K, lda, ldb, ldc, a_gather, b_gather, scratch)
    "head": (192, 12, 64, 16, 64, 64, (0, 0, 0), (64, 66, 2), "64M"),
    "patch_embed": (192, 64, 12, 64, 16, 12, (64, 66, 2), (0, 0, 0), "64M"),
    "m33": (33, 64, 16, 64, 16, 20, (0, 0, 0), (0, 0, 0), "64M"),
    "split": (1100, 64, 128, 64, 128, 128, (0, 0, 0), (0, 0, 0), "64M"),
    "split_noscratch": (1100, 64, 128, 64, 128, 128, (0, 0, 0), (0, 0, 0), None),
    "k1024": (517, 20, 1024, 24, 1024, 1028, (0, 0, 0), (0, 0, 0), "64M"),
}


@pytest.fixture(scope="module")
def wgrad_data():
    data = {}
    for i, (name, (M, N, K, lda, ldb, ldc, ag, bg, _)) in enumerate(WGRAD_CASES.items()):
        g = gen(100 + i)
        A, av, _ = gathered(g, M, N, lda, ag, BF)
        B, bv, _ = gathered(g, M, K, ldb, bg, BF)
        a64, b64 = av.double(), bv.double()
        data[name] = dict(A=A.to(DEV), B=B.to(DEV), dw=a64.t() @ b64, dw_abs=a64.abs().t() @ b64.abs(),
                          db=a64.sum(0), db_abs=a64.abs().sum(0), C0=randn(g, N, ldc), b0=randn(g, N + 4))
    return data


@pytest.mark.parametrize("tile", [0, 128, 256])
@pytest.mark.parametrize("name", list(WGRAD_CASES))
def test_wgrad_gather_bias(lib, wgrad_data, scratch64, name, tile):
    M, N, K, lda, ldb, ldc, ag, bg, sc = WGRAD_CASES[name]
    d = wgrad_data[name]
    scratch = scratch64 if sc else None
    lib.check(lib.load().pdm_set_wgrad_tile(tile))
    try:
        for accumulate in (0, 1):
            for bias_acc in (0, 1):
                C = (d["C0"].clone() if accumulate else torch.full((N, ldc), SENT)).to(DEV)
                bias = (d["b0"].clone() if bias_acc else torch.full((N + 4,), SENT)).to(DEV)
                C_before, b_before = C.clone(), bias.clone()
                lib.wgrad_gather(d["A"], lda, d["B"], ldb, C, ldc, M, N, K, ag, bg, accumulate=accumulate,
                                 bias_out=bias, bias_acc=bias_acc, scratch=scratch)
                what = f"{name} tile {tile} acc {accumulate} bias_acc {bias_acc}"
                c0 = d["C0"][:, :K].double() if accumulate else torch.zeros(N, K, dtype=torch.float64)
                ref = d["dw"] + c0
                hold("wgrad dW", C[:, :K], ref, (M + accumulate + 2) * U * (d["dw_abs"] + c0.abs()), what)
                r = rel(C[:, :K], ref)
                assert r < 1e-5, (what, r)
                assert same_bits(C[:, K:], C_before[:, K:]), what + ": dW padding columns touched"
                bb = d["b0"][:N].double() if bias_acc else torch.zeros(N, dtype=torch.float64)
                hold("wgrad bias", bias[:N], d["db"] + bb, (M + bias_acc + 2) * U * (d["db_abs"] + bb.abs()), what)
                assert same_bits(bias[N:], b_before[N:]), what + ": past the bias"
    finally:
        lib.check(lib.load().pdm_set_wgrad_tile(0))


def test_wgrad_bias_needs_n_multiple_of_4(lib):
    A = torch.zeros(32, 8, dtype=BF, device=DEV)
    C = torch.zeros(6, 8, device=DEV)
    with pytest.raises(ValueError):
        lib.wgrad_gather(A, 8, A, 8, C, 8, 32, 6, 8, bias_out=torch.zeros(8, device=DEV))
    lib.wgrad_gather(A, 8, A, 8, C, 8, 32, 6, 8)          # without the bias N = 6 is fine
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------
# column sums

def _colsum_case(lib, g, rows, ncols, ld, bf, gather, scratch, what):
    x, vals, _ = gathered(g, rows, ncols, ld, gather, BF if bf else torch.float32)
    v = vals.double()
    d0 = randn(g, ncols + 4)
    xd = x.to(DEV)
    for accumulate in (0, 1):
        dst = (d0.clone() if accumulate else torch.full((ncols + 4,), SENT)).to(DEV)
        before = dst.clone()
        lib.colsum(xd, ld, rows, ncols, dst, gather, accumulate=accumulate, scratch=scratch)
        p = d0[:ncols].double() if accumulate else torch.zeros(ncols, dtype=torch.float64)
        hold("colsum", dst[:ncols], v.sum(0) + p, (rows + accumulate + 2) * U * (v.abs().sum(0) + p.abs()),
             f"{what} acc {accumulate}")
        assert same_bits(dst[ncols:], before[ncols:]), what + ": past dst"


@pytest.mark.parametrize("bf", [0, 1])
@pytest.mark.parametrize("ncols", [4, 1028])
@pytest.mark.parametrize("rows", [1, 16, 17, 257])
def test_colsum(lib, rows, ncols, bf, ):
    scratch = torch.empty(1 << 18, dtype=torch.float32, device=DEV)       # 1 MiB: 16-row chunks, 257 rows = 3 passes
    _colsum_case(lib, gen(rows * 7 + ncols + bf), rows, ncols, ncols + 4, bf, (0, 0, 0), scratch,
                 f"rows {rows} ncols {ncols} bf16 {bf}")


@pytest.mark.parametrize("bf", [0, 1])
def test_colsum_special_calls(lib, bf):
    big = torch.empty(1 << 18, dtype=torch.float32, device=DEV)
    g = gen(40 + bf)
    _colsum_case(lib, g, 3, 66 * 64, 66 * 64, bf, (0, 0, 0), big, "pos_embed (ld = ncols = L D)")
    _colsum_case(lib, g, 192, 64, 64, bf, (64, 66, 2), big, "gather (64, 66, 2)")
    small = torch.empty(2 * 4 * 1028, dtype=torch.float32, device=DEV)    # fewer, longer chunks: 4 x 65 rows, then 1
    _colsum_case(lib, g, 257, 1028, 1028, bf, (0, 0, 0), small, "scratch 2*4*1028*4 B")
    _colsum_case(lib, g, 257, 1028, 1032, bf, (0, 0, 0), None, "NULL scratch (one pass)")


# ---------------------------------------------------------------------------------------------------------------
# LayerNorm backward (general form) and forward with a row gather

def _ln_inputs(g, rows, D, gather, ld):
    idx = R.gather_index(rows, *gather)
    phys = int(idx.max()) + 1 + (2 if gather[0] else 0)
    x = torch.full((phys, ld), NAN)
    xv = randn(g, rows, D, scale=3.0) + 1.0
    x[idx, :D] = xv
    gamma = 0.5 + torch.rand(D, generator=g)
    return x, xv, idx, phys, gamma


LN_SHAPES = [(D, rows) for D in (4, 64, 1152, 2048) for rows in (1, 7)] + [(64, 4100)]


@pytest.mark.parametrize("dh_bf16", [0, 1])
@pytest.mark.parametrize("D,rows", LN_SHAPES)
def test_layernorm_backward_rows(lib, D, rows, dh_bf16):
    g = gen(D * 3 + rows + dh_bf16)
    big = torch.empty(1 << 20, dtype=torch.float32, device=DEV)            # 4 MiB: nblk = min(1024, ceil(rows / 4))
    one = torch.empty(10 * D, dtype=torch.float32, device=DEV)             # 40 D bytes: nblk = 1, every block loops
    # (gather, dbeta right after dgamma, accumulate_params, accumulate, scratch)
    variants = [((0, 0, 0), 1, 0, 0, big), ((9, 11, 2), 0, 1, 1, big), ((0, 0, 0), 0, 0, 1, one),
                ((9, 11, 2), 1, 1, 0, one)]
    for gather, contig, accp, acc, scratch in variants:
        ld = D + 8 if gather[0] else D
        x, xv, idx, phys, gamma = _ln_inputs(g, rows, D, gather, ld)
        lddh = D + 4 if gather[0] else D
        dh_full = torch.full((rows, lddh), NAN)
        dhv = randn(g, rows, D).to(BF if dh_bf16 else torch.float32)
        dh_full[:, :D] = dhv.float()
        dh_full = dh_full.to(dhv.dtype)
        dx0 = randn(g, phys, ld)
        dx = (dx0.clone() if acc else torch.full((phys, ld), SENT)).to(DEV)
        dxb = torch.full((phys, ld), SENT, dtype=BF, device=DEV)
        pg0 = randn(g, 3 * D + 4)
        pbuf = (pg0.clone() if accp else torch.full((3 * D + 4,), SENT)).to(DEV)
        dgamma = pbuf[:D]
        dbeta = pbuf[D:2 * D] if contig else pbuf[2 * D + 4: 3 * D + 4]
        dx_before, dxb_before, p_before = dx.clone(), dxb.clone(), pbuf.clone()
        lib.layernorm_backward_rows(x.to(DEV), ld, dh_full.to(DEV), lddh, gamma.to(DEV), dx, ld, dxb, dgamma, dbeta,
                                    rows, D, scratch, gather, accumulate=acc, accumulate_params=accp)
        what = f"D {D} rows {rows} dh_bf16 {dh_bf16} gather {gather} contig {contig} accp {accp} acc {acc}"
        rdx, rdg, rdb = R.layernorm_backward_ref(xv, dhv, gamma)
        if acc:
            rdx = rdx + dx0[idx, :D].double()
        beta_off = D if contig else 2 * D + 4
        pg = pg0[:D].double() if accp else 0.0
        pb = pg0[beta_off:beta_off + D].double() if accp else 0.0
        dxo = dx.cpu()
        for name, out, ref in (("dx", dxo[idx, :D], rdx), ("dgamma", dgamma, rdg + pg), ("dbeta", dbeta, rdb + pb)):
            r = rel(out, ref)
            WORST[f"ln_bwd {name} rel-L2 / 1e-5"] = max(WORST.get(f"ln_bwd {name} rel-L2 / 1e-5", 0.0), r / 1e-5)
            print(f"ln_bwd {what}: {name} rel-L2 = {r:.3e}")
            assert r < 1e-5, (what, name, r)
        # dbeta is a plain column sum of dh
        hold("ln_bwd dbeta", dbeta, rdb + pb, (rows + accp + 2) * U * (dhv.double().abs().sum(0) + abs(pb)), what)
        # the bf16 copy is a cast of what was stored; rows the gather skips and padding columns stay as they were
        assert same_bits(dxb.cpu()[idx, :D], dxo[idx, :D].to(BF)), what + ": dxb != bf16(dx)"
        keep = torch.ones(phys, ld, dtype=torch.bool)
        keep[idx, :D] = False
        assert torch.equal(bits(dxo)[keep], bits(dx_before.cpu())[keep]), what + ": dx outside the rows"
        assert torch.equal(bits(dxb.cpu())[keep], bits(dxb_before.cpu())[keep]), what + ": dxb outside the rows"
        pk = torch.ones(3 * D + 4, dtype=torch.bool)
        pk[:D] = False
        pk[beta_off:beta_off + D] = False
        assert torch.equal(bits(pbuf.cpu())[pk], bits(p_before.cpu())[pk]), what + ": outside dgamma / dbeta"


def test_layernorm_backward_rows_rejects(lib):
    big = torch.empty(1 << 16, dtype=torch.float32, device=DEV)

    def call(D, scratch, rows=7):
        x = torch.zeros(rows, D, device=DEV)
        p = torch.zeros(2 * D, device=DEV)
        lib.layernorm_backward_rows(x, D, x, D, torch.ones(D, device=DEV), x.clone(), D, None, p[:D], p[D:], rows, D,
                                    scratch)
    for D, scratch in ((2052, big), (66, big), (64, big[: 10 * 64 - 8]), (64, big[:8])):
        with pytest.raises(ValueError):
            call(D, scratch)
    call(64, big[: 10 * 64])
    torch.cuda.synchronize()


@pytest.mark.parametrize("D,rows", LN_SHAPES)
def test_layernorm_rows_gather(lib, D, rows):
    """y = bf16(gamma xhat + beta).  fp32 bound: the mean carries (D + 1) u A (A = mean |x|), so xhat carries
    |xhat| (D + 11) / 2 u from rstd and its own roundings plus (D + 1) u A rstd from the mean; the affine adds
    2 u (|gamma xhat| + |beta|): within (D + 16) u (|gamma| (|xhat| + A rstd) + |beta|).  Plus 0.5 bf16 ulp."""
    g = gen(D + rows)
    for gather in ((rows, 0, 0), (9, 11, 2)):
        ld = D + 8 if gather[1] else D
        x, xv, idx, phys, gamma = _ln_inputs(g, rows, D, gather, ld)
        beta = randn(g, D)
        ldy = D + 4
        y = torch.full((rows + 1, ldy), SENT, dtype=BF, device=DEV)
        before = y.clone()
        lib.layernorm_rows(x.to(DEV), ld, gamma.to(DEV), beta.to(DEV), y, ldy, rows, D, gather)
        ref = R.layernorm_ref(xv, gamma, beta)
        x64 = xv.double()
        rstd = 1.0 / torch.sqrt(x64.var(-1, unbiased=False, keepdim=True) + 1e-5)
        xhat = (x64 - x64.mean(-1, keepdim=True)) * rstd
        A = x64.abs().mean(-1, keepdim=True)
        bound = (D + 16) * U * (gamma.double() * (xhat.abs() + A * rstd) + beta.double().abs()) + half_ulp_bf16(ref)
        hold("layernorm fwd", y[:rows, :D], ref, bound, f"D {D} rows {rows} gather {gather}")
        yc = y.cpu()
        assert same_bits(yc[:rows, D:], before.cpu()[:rows, D:]) and same_bits(yc[rows:], before.cpu()[rows:])


def test_layernorm_rows_rejects(lib):
    for D in (2052, 66):
        x = torch.zeros(4, D, device=DEV)
        with pytest.raises(ValueError):
            lib.layernorm_rows(x, D, x[0], x[0], torch.zeros(4, D, dtype=BF, device=DEV), D, 4, D, (4, 0, 0))


# ---------------------------------------------------------------------------------------------------------------
# GELU over every finite bf16 value

@pytest.fixture(scope="module")
def all_bf16():
    pat = torch.arange(65536, dtype=torch.int32)
    pat = pat[(pat & 0x7F80) != 0x7F80]
    assert pat.numel() == 65280
    return pat.to(torch.int16).view(BF)


def test_gelu_forward_all_bf16(lib, all_bf16):
    u = all_bf16.to(DEV)
    g = torch.full((u.numel() + 8,), SENT, dtype=BF, device=DEV)
    lib.gelu_forward(u, g, u.numel())
    out = g[: u.numel()].cpu()
    assert not torch.isnan(out.float()).any() and same_bits(g[u.numel():].cpu(), torch.full((8,), SENT, dtype=BF))
    ref = R.gelu_ref(all_bf16)
    hold("gelu fwd", out, ref, half_ulp_bf16(ref) + all_bf16.double().abs() * 2.0 ** -23, "65280 values")


@pytest.mark.parametrize("dg", [1.0, -3.5])
def test_gelu_backward_all_bf16(lib, all_bf16, dg):
    u = all_bf16.to(DEV)
    d = torch.full((u.numel() + 8,), dg, dtype=BF, device=DEV)
    lib.gelu_backward(d, u, u.numel())
    out = d[: u.numel()].cpu()
    assert not torch.isnan(out.float()).any() and same_bits(d[u.numel():].cpu(), torch.full((8,), dg, dtype=BF))
    ref = dg * R.gelu_grad_ref(all_bf16)
    hold("gelu bwd", out, ref, half_ulp_bf16(ref) + abs(dg) * (1 + all_bf16.double().abs()) * 2.0 ** -23, f"dg {dg}")


def test_gelu_rejects_n_not_multiple_of_8(lib):
    u = torch.zeros(16, dtype=BF, device=DEV)
    with pytest.raises(ValueError):
        lib.gelu_forward(u, u.clone(), 12)
    with pytest.raises(ValueError):
        lib.gelu_backward(u.clone(), u, 12)


# ---------------------------------------------------------------------------------------------------------------
# LSimple

@pytest.mark.parametrize("tanh_bwd", [0, 1])
@pytest.mark.parametrize("per", [5, 256, 1000, 3072])
def test_lsimple(lib, per, tanh_bwd):
    for B in (1, 3):
        for gscale in (1.0 / B, 0.37):
            g = gen(per + B + tanh_bwd)
            pred = torch.tanh(randn(g, B, per, scale=3.0).double()).float() if tanh_bwd else randn(g, B, per)
            tgt = randn(g, B, per)
            loss = torch.full((B + 2,), SENT, device=DEV)
            dp = torch.full((B * per + 8,), SENT, device=DEV)
            lib.lsimple(pred.to(DEV), tgt.to(DEV), loss, dp, B, per, gscale, tanh_bwd)
            gs32 = float(torch.tensor(gscale, dtype=torch.float32))       # the scale the kernel receives
            rl, rd, terms = R.lsimple_ref(pred, tgt, gs32, tanh_bwd)
            what = f"per {per} B {B} gscale {gscale:.3f} tanh {tanh_bwd}"
            hold("lsimple loss", loss[:B], rl, (per + 2) * U * terms.mean(-1), what)
            kd = (-2.0 * gs32 / per) * (tgt.double() - pred.double())
            hold("lsimple dpred", dp[: B * per].view(B, per), rd, 2.0 ** -21 * rd.abs() + 2.0 ** -23 * kd.abs(), what)
            assert float(loss[B:].min()) == SENT == float(loss[B:].max()) and bool((dp[B * per:] == SENT).all())


# ---------------------------------------------------------------------------------------------------------------
# final_layer conv3x3 backward

@pytest.mark.parametrize("B,C,H,W", [(2, 3, 5, 5), (1, 4, 8, 6), (3, 8, 4, 4)])
def test_conv3x3_backward(lib, B, C, H, W):
    import torch.nn.functional as F
    g = gen(B * 100 + C)
    dout, x, w = randn(g, B, C, H, W), randn(g, B, C, H, W), randn(g, C, C, 3, 3, scale=0.3)
    din = torch.full((B * C * H * W + 4,), SENT, device=DEV)
    dw = torch.full((C * C * 9 + 4,), SENT, device=DEV)
    db = torch.full((C + 4,), SENT, device=DEV)
    lib.conv3x3_backward(dout.to(DEV), x.to(DEV), w.to(DEV), din, dw, db)
    rdin, rdw, rdb = R.conv3x3_backward_ref(dout, x, w)
    a_din = F.conv_transpose2d(dout.double().abs(), w.double().abs(), padding=1)
    a_dw = torch.nn.grad.conv2d_weight(x.double().abs(), w.shape, dout.double().abs(), padding=1)
    what = f"B {B} C {C} {H}x{W}"
    hold("conv3x3 bwd din", din[:-4].view(B, C, H, W), rdin, (9 * C + 2) * U * a_din, what)
    hold("conv3x3 bwd dw", dw[:-4].view(C, C, 3, 3), rdw, (B * H * W + 2) * U * a_dw, what)
    hold("conv3x3 bwd db", db[:-4], rdb, (B * H * W + 2) * U * dout.double().abs().sum((0, 2, 3)), what)
    for t in (din, dw, db):
        assert bool((t[-4:] == SENT).all()), what


# ---------------------------------------------------------------------------------------------------------------
# decoder_pred + unpatchify, forward and backward

HEAD_SHAPES = [(C, 2, H, W) for C in (3, 4, 8) for (H, W) in ((6, 6), (8, 12))] + [(4, 4, 8, 12)]


@pytest.mark.parametrize("D", [64, 72, 256])
@pytest.mark.parametrize("C,p,H,W", HEAD_SHAPES)
def test_head_forward(lib, C, p, H, W, D):
    B, h, w = 3, H // p, W // p
    N, P = h * w, p * p * C
    P_pad = (P + 15) & ~15
    g = gen(C * 1000 + p * 100 + H + D)
    wt = torch.full((P_pad, D), 1e4)          # rows >= P belong to the padding: their products are never stored
    wt[:P] = randn(g, P, D, scale=D ** -0.5)
    wt = wt.to(BF)
    bias = randn(g, P)
    for gs, off in ((N, 0), (N + 5, 3)):
        ld = D + 8 if off else D
        tok = randn(g, B, N, D).to(BF)
        x = torch.full((B * gs + off + 2, ld), NAN)
        idx = R.gather_index(B * N, N, gs, off)
        x[idx, :D] = tok.reshape(B * N, D).float()
        xd = x.to(BF).to(DEV)
        for act_tanh in (0, 1):
            out = torch.full((B * C * H * W + 4,), SENT, device=DEV)
            lib.head_forward(xd, ld, gs, off, wt.to(DEV), bias.to(DEV), out, B, D, C, p, H, W, P_pad, act_tanh)
            ref = R.head_ref(tok, wt[:P], bias, C, h, w, act_tanh)
            lin_abs = tok.double().abs() @ wt[:P].double().abs().t() + bias.double().abs()
            bound = (D + 1 + 2) * U * R.unpatchify_ref(lin_abs, C, h, w)
            if act_tanh:            # tanh is 1-Lipschitz; tanhf itself within 2 ulp of a value <= 1
                bound = bound + 2.0 ** -22
            hold("head fwd", out[:-4].view(B, C, H, W), ref, bound, f"C {C} p {p} {H}x{W} D {D} gs {gs} tanh {act_tanh}")
            assert bool((out[-4:] == SENT).all())


@pytest.mark.parametrize("D", [64, 260])
@pytest.mark.parametrize("C,p,H,W", HEAD_SHAPES)
def test_head_backward(lib, C, p, H, W, D):
    B, h, w = 3, H // p, W // p
    N, P = h * w, p * p * C
    P_pad = (P + 15) & ~15
    g = gen(C * 1000 + p * 100 + H + D + 1)
    dpre, wt = randn(g, B, C, H, W), randn(g, P, D, scale=0.2)
    dtok = torch.full((B * N + 1, P_pad), SENT, dtype=BF, device=DEV)
    dx = torch.full((B * N + 1, D), SENT, device=DEV)
    lib.head_backward(dpre.to(DEV), wt.to(DEV), dtok, dx, B, D, C, p, H, W, P_pad)
    rtok, rdx = R.head_backward_ref(dpre, wt, C, p)
    want = torch.zeros(B * N, P_pad, dtype=BF)
    want[:, :P] = rtok.reshape(B * N, P).float().to(BF)      # fp32 values: the double round trip is exact
    assert same_bits(dtok[:-1].cpu(), want), "dtok != bf16 of the gathered gradient, zero padded"
    bound = (P + 2) * U * (rtok.abs() @ wt.double().abs())
    hold("head bwd dx", dx[:-1].view(B, N, D), rdx, bound, f"C {C} p {p} {H}x{W} D {D}")
    assert bool((dx[-1] == SENT).all()) and bool((dtok[-1].float() == float(torch.tensor(SENT).to(BF))).all())


def test_head_rejects(lib):
    z = torch.zeros(64, 64, dtype=BF, device=DEV)
    f = torch.zeros(4096, device=DEV)
    with pytest.raises(ValueError):       # P = 4 * 4 * 5 = 80 > 64
        lib.head_forward(z, 64, 9, 0, z, f, f, 1, 64, 5, 4, 12, 12, 80)
    with pytest.raises(ValueError):
        lib.head_backward(f, f, z, f, 1, 64, 5, 4, 12, 12, 80)
    with pytest.raises(ValueError):       # 6 x 6 is not divisible by p = 4
        lib.head_forward(z, 64, 1, 0, z, f, f, 1, 64, 4, 4, 6, 6, 64)
    with pytest.raises(ValueError):       # D % 8
        lib.head_forward(z, 64, 9, 0, z, f, f, 1, 60, 4, 2, 6, 6, 16)


# ---------------------------------------------------------------------------------------------------------------
# token assembly

@pytest.mark.parametrize("D", [64, 260])
@pytest.mark.parametrize("K", [12, 16, 32, 64, 48])
def test_assemble(lib, K, D):
    p, H, B, ncls, nctx = 2, 10, 3, 7, 2
    C, npatch = K // 4, 25
    ld = D + 4
    g = gen(K * 10 + D)
    img = randn(g, B, C, H, H)
    pw, pb = randn(g, D, K, scale=K ** -0.5), randn(g, D)
    t = torch.tensor([0.0, 0.5, 999.0])
    y = torch.tensor([0, ncls - 1, 3])
    lab, temb, ctx = randn(g, ncls, D), randn(g, B, D), randn(g, B, nctx, D)
    dev = lambda v: v.to(DEV)   # noqa: E731
    pv = R.patch_vectors_ref(img.double(), p)
    patch_abs = pv.abs() @ pw.double().abs().t() + pb.double().abs()

    def run(extras, Lbuf, row_off, **kw):
        L = extras + npatch
        pos = randn(g, L, D)
        out = torch.full((B, Lbuf, ld), SENT, device=DEV)
        before = out.clone()
        view = out.view(-1)[row_off * ld:]
        lib.assemble(dev(img), p, dev(pw), dev(pb), dev(pos), view, ld, D, Lbuf, extras,
                     **{k: (dev(v) if torch.is_tensor(v) else v) for k, v in kw.items()})
        o = out.cpu()[:, row_off:row_off + L]
        keep = torch.ones(B, Lbuf, ld, dtype=torch.bool)
        keep[:, row_off:row_off + L, :D] = False
        assert torch.equal(bits(out.cpu())[keep], bits(before.cpu())[keep]), "assemble wrote outside its rows"
        return o[..., :D], pos

    def check_patches(o, pos, extras, what):
        ref = R.patch_embed_ref(img, pw, pb, p) + pos[extras:].double()
        hold("assemble patches", o[:, extras:], ref, (K + 2 + 2) * U * (patch_abs + pos[extras:].double().abs()),
             f"K {K} D {D} {what}")

    def check_time(o, pos, row, what):
        emb, args = R.timestep_embedding_ref(t, D)
        b = 2.0 ** -22 + args.abs() * 2.0 ** -21
        hold("assemble time row", o[:, row], emb + pos[row].double(), torch.cat([b, b], -1), f"K {K} D {D} {what}")

    # libs/uvit.py, unconditional: [time][patches]
    o, pos = run(1, 1 + npatch, 0, t=t, time_row=0)
    check_time(o, pos, 0, "uncond")
    check_patches(o, pos, 1, "uncond")
    # class-conditional: [label][time][patches], labels 0 and num_classes - 1
    o, pos = run(2, 2 + npatch, 0, t=t, time_row=1, y=y, label_emb=lab, label_row=0)
    assert same_bits(o[:, 0].contiguous(), lab[y] + pos[0]), "label row != label_emb[y] + pos"
    check_time(o, pos, 1, "cond")
    check_patches(o, pos, 2, "cond")
    # t2i image stream: [time_emb][context x nctx][patches]
    o, pos = run(1 + nctx, 1 + nctx + npatch, 0, time_emb=temb, time_row=0, ctx_tokens=ctx, ctx_row=1)
    assert same_bits(o[:, 0].contiguous(), temb + pos[0]), "time row != time_emb + pos"
    assert same_bits(o[:, 1:1 + nctx].contiguous(), ctx + pos[1:1 + nctx]), "context rows != ctx + pos"
    check_patches(o, pos, 1 + nctx, "t2i")
    # t2i mask stream: the patch rows alone, written behind the image rows of a longer sequence
    o, pos = run(0, 9 + npatch, 9)
    check_patches(o, pos, 0, "mask rows")


# ---------------------------------------------------------------------------------------------------------------
# data movement: bit-equal to torch

@pytest.mark.parametrize("C,p,ldp,H,W", [(3, 2, 16, 6, 10), (4, 4, 64, 8, 12), (8, 2, 32, 4, 6)])
def test_patchify(lib, C, p, ldp, H, W):
    B = 2
    img = randn(gen(C + p), B, C, H, W)
    N = (H // p) * (W // p)
    pv = torch.full((B * N + 1, ldp), SENT, dtype=BF, device=DEV)
    lib.patchify(img.to(DEV), pv, p, ldp)
    want = torch.zeros(B * N, ldp, dtype=BF)
    want[:, : C * p * p] = R.patch_vectors_ref(img, p).reshape(B * N, -1).to(BF)
    assert same_bits(pv[:-1].cpu(), want)
    assert bool((pv[-1].float() == float(torch.tensor(SENT).to(BF))).all())


@pytest.mark.parametrize("acc", [0, 1])
def test_rows_add_cast_t2i_calls(lib, acc):
    """The three calls of the t2i backward at Lx 9, Lm 14 (5 patches), D 8, batch 2."""
    Lx, Lm, D, B = 9, 14, 8, 2
    npt = Lm - Lx
    g = gen(77 + acc)
    calls = [("mask head -> mask rows", (npt, Lm, Lx), B * Lm, (0, 0, 0), B * npt, B * npt),
             ("injection -> image rows of the mask stream", (Lx, Lm, 0), B * Lm, (0, 0, 0), B * Lx, B * Lx),
             ("mask stream's image rows -> x", (0, 0, 0), B * Lx, (Lx, Lm, 0), B * Lm, B * Lx)]
    for what, dg, drows, sg, srows, rows in calls:
        src = torch.full((srows, D), NAN)
        si, di = R.gather_index(rows, *sg), R.gather_index(rows, *dg)
        src[si] = randn(g, rows, D)
        dst0 = randn(g, drows + 1, D)
        dst, dstb = dst0.clone().to(DEV), torch.full((drows + 1, D), SENT, dtype=BF, device=DEV)
        lib.rows_add_cast(dst, dstb, dg, src.to(DEV), sg, rows, D, accumulate=acc)
        want = dst0.clone()
        want[di] = dst0[di] + src[si] if acc else src[si]
        assert same_bits(dst.cpu(), want), what
        wb = torch.full((drows + 1, D), SENT, dtype=BF)
        wb[di] = want[di].to(BF)
        assert same_bits(dstb.cpu(), wb), what


@pytest.mark.parametrize("with_add", [0, 1])
def test_add_cast(lib, with_add):
    n = 4 * (256 * 3 + 5)
    g = gen(5 + with_add)
    dx0, add = randn(g, n + 4), randn(g, n)
    dx, dxb = dx0.clone().to(DEV), torch.full((n + 4,), SENT, dtype=BF, device=DEV)
    lib.add_cast(dx, add.to(DEV) if with_add else None, dxb, n)
    want = dx0.clone()
    if with_add:
        want[:n] = dx0[:n] + add
    assert same_bits(dx.cpu(), want)
    wb = torch.full((n + 4,), SENT, dtype=BF)
    wb[:n] = want[:n].to(BF)
    assert same_bits(dxb.cpu(), wb)
    with pytest.raises(ValueError):
        lib.add_cast(dx, None, dxb, 6)


def test_transpose_bf16(lib):
    g = gen(6)
    for N in (4, 60, 64, 68, 132):
        for K in (4, 60, 64, 68, 132):
            w = randn(g, N, K)
            wt = torch.full((K * N + 4,), SENT, dtype=BF, device=DEV)
            lib.transpose_bf16(w.to(DEV), wt, N, K)
            assert same_bits(wt[:-4].cpu().view(K, N), w.t().contiguous().to(BF)), (N, K)
            assert bool((wt[-4:].float() == float(torch.tensor(SENT).to(BF))).all()), (N, K)
    w = torch.zeros(8, 8, device=DEV)
    for N, K in ((6, 8), (8, 6)):
        with pytest.raises(ValueError):
            lib.transpose_bf16(w, torch.zeros(64, dtype=BF, device=DEV), N, K)


@pytest.mark.parametrize("row", [0, 1])
def test_label_scatter(lib, row):
    B, D, L, ncls = 5, 260, 3, 8
    y = torch.tensor([2, 2, 0, 2, 6])
    g = gen(8 + row)
    dx, dlab0 = randn(g, B * L, D), randn(g, ncls, D)
    dlab = dlab0.clone().to(DEV)
    lib.label_scatter(dx.to(DEV), L, row, D, y.to(DEV), dlab, B)
    rows = dx.view(B, L, D)[:, row].double()
    ref, mag = dlab0.double().clone(), dlab0.double().abs().clone()
    ref.index_add_(0, y, rows)
    mag.index_add_(0, y, rows.abs())
    hold("label_scatter", dlab, ref, (3 + 2) * U * mag, f"row {row}")
    out = dlab.cpu()
    for c in (1, 3, 4, 5, 7):
        assert same_bits(out[c], dlab0[c]), f"class {c} touched"
    for b, c in ((2, 0), (4, 6)):               # a single add: bit-equal
        assert same_bits(out[c], dlab0[c] + dx.view(B, L, D)[b, row])


# ---------------------------------------------------------------------------------------------------------------
# AdamW + EMA + the bf16 copies, on a tiny_uvit_train trainer's flat buffers

@pytest.fixture(scope="module")
def trainer():
    from panopticdiffusionmodels_amd import configs, weights
    from panopticdiffusionmodels_amd.train import HipTrainState
    full = configs.get_config("tiny_uvit_train")
    st = HipTrainState(full["nnet"], DEV)
    sd = weights.nnet_state_dict(full["nnet"], seed=11, init="random")
    st.load_state_dict(sd)
    return st, sd


@pytest.mark.parametrize("wd", [0.0, 0.03])
@pytest.mark.parametrize("step", [1, 2, 10, 1000])
def test_adamw_steps(lib, trainer, step, wd):
    st, sd = trainer
    n = st.n
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))   # noqa: E731  the hyperparameters the kernel receives
    lr, b1, b2, eps, rate = f32(2e-4), f32(0.9), f32(0.999), f32(1e-8), f32(0.9999)
    wdf = f32(wd)
    for use_g2 in (0, 1):
        for use_ema in (0, 1):
            g = gen(step * 10 + use_g2 * 2 + use_ema + int(wd * 100))
            P0, G, G2, M0, E0 = (randn(g, n) for _ in range(5))
            M0 = M0 * 0.3
            V0 = torch.rand(n, generator=g)
            st.P.copy_(P0)
            st.G.copy_(G)
            M, V, E, g2 = M0.to(DEV), V0.to(DEV), E0.to(DEV), G2.to(DEV)
            lib.check(st.lib.pdm_train_adamw(st.h, lib.ptr(M), lib.ptr(V), lib.ptr(E) if use_ema else None,
                                             lib.ptr(g2) if use_g2 else None, lr, b1, b2, eps, wdf, step, rate,
                                             lib.stream_ptr(st.device)), "pdm_train_adamw")
            gr = (G + G2).double() if use_g2 else G.double()   # the lanes' gradients: one fp32 add, then the moments
            rp, rm, rv, re, upd = R.adamw_ema_ref(P0, gr, M0, V0, E0 if use_ema else None, step, lr, (b1, b2), eps,
                                                  wdf, rate)
            what = f"step {step} wd {wd} g2 {use_g2} ema {use_ema}"
            hold("adamw m", M, rm, 2.0 ** -23 * ((b1 * M0.double()).abs() + ((1 - b1) * gr).abs()), what)
            hold("adamw v", V, rv, 2.0 ** -23 * ((b2 * V0.double()).abs() + ((1 - b2) * gr * gr).abs()), what)
            pb = 2.0 ** -23 * rp.abs() + 2.0 ** -21 * upd.abs()
            hold("adamw p", st.P, rp, pb, what)
            if use_ema:
                # ema = rate ema + (1 - rate) p, from the kernel's own fp32 p: two products and a sum, each within
                # u of itself, i.e. 2^-23 (|rate ema| + |(1 - rate) p|) like m and v, plus (1 - rate) times p's bound.
                # Relative to the new ema alone (2^-23 |ema| + 2^-21 |update|) no fp32 evaluation can hold where the
                # two terms cancel (|ema| ~ 1e-4 |p|, opposite signs: about one element in 1e5): that figure is
                # printed, not asserted.
                terms = (rate * E0.double()).abs() + ((1 - rate) * rp).abs()
                hold("adamw ema", E, re, 2.0 ** -23 * terms + (1 - rate) * pb, what)
                lit = (E.cpu().double() - re).abs() / (2.0 ** -23 * re.abs() + 2.0 ** -21 * upd.abs())
                WORST["adamw ema, relative to |ema| alone (not asserted)"] = max(
                    WORST.get("adamw ema, relative to |ema| alone (not asserted)", 0.0), float(lit.max()))
                print(f"adamw ema {what}: {int((lit > 1).sum())} of {n} elements past 2^-23 |ema| + 2^-21 |update|")
            else:
                assert same_bits(E.cpu(), E0), what + ": ema touched"
            # the bf16 working copy over the whole buffer, and every block Linear's transposed copy
            assert same_bits(st.WB, st.P.to(BF)), what + ": bf16 working copy"
            off_t = 0
            lin = (".skip_linear.weight", ".attn.qkv.weight", ".attn.proj.weight", ".mlp.fc1.weight",
                   ".mlp.fc2.weight")
            nlin = 0
            for k, (off, numel) in st.index.items():
                if k.endswith(lin) and k.split(".")[0] in ("in_blocks", "mid_block", "out_blocks"):
                    N, K = sd[k].shape
                    W = st.P[off:off + numel].view(N, K)
                    assert same_bits(st.WT[off_t:off_t + numel].view(K, N), W.t().contiguous().to(BF)), (what, k)
                    off_t += (numel + 63) // 64 * 64
                    nlin += 1
            assert nlin > 0 and off_t == st.WT.numel(), (nlin, off_t, st.WT.numel())
    st.load_state_dict(sd)
