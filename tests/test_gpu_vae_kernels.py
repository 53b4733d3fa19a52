"""The KL-f8 autoencoder's kernels one by one (include/pdm.h pdm_vae_*, pdm_gemm_*_gn): each HIP kernel against plain
torch in float64 on the same rounded operands, at the smallest shapes that reach every code path.

Bounds (the project's precedents, tests/test_gpu_kernels.py / test_gpu_train.py):
  * bf16 operands with fp32 accumulation, or fp32 arithmetic, vs float64: rel-L2 < 1e-5 (test_wgrad_vs_torch,
    test_stage_epilogue, the LayerNorm-partials tests) -- decoder conv_in, both conv_out kernels, encoder conv_in, the
    encoder tail, the products of the GroupNorm-partials GEMMs;
  * one bf16 rounding of an fp32 result: every element within one bf16 ulp of the float64 value, 2e-5 absolute floor
    (test_gelu_activation_exactness; the floor covers the fp32 cancellation in x * a + o, ~3 * 2^-24 * (|x a| + |o|))
    -- the GroupNorm apply and the softmax;
  * GroupNorm (mean, rstd): |d mean| <= 1e-6 * rms of the group (= |mean| to 1 % once |mean| / std = 8, and the only
    scale there is when the mean is ~0), |d rstd| <= 1e-5 * rstd.  The kernels keep fp32 per-thread sums of <= 128
    values merged in fp64; var = E[x^2] - mean^2 in fp64 then loses ~n 2^-24 (1 + r^2) / 2 at worst (r = |mean| / std);
    a CPU emulation of that order gave 4e-7 at r = 8: 1e-5 leaves 25x;
  * GroupNorm partials of a GEMM epilogue, EVERY entry: |d sum| <= 1e-5 * sum |x|, |d sumsq| <= 1e-5 * sumsq of the
    values the kernel itself stored;
  * data movement (transpose, downsample gather): bit-equal.
A bf16 GEMM output is compared at rel-L2 < 2^-8: one rounding is <= 2^-9 relative per element, so rel-L2 <= 2^-9 plus
the fp32 accumulation's ~1e-6.

Inputs are structured so that an indexing bug cannot hide: every (image, group) has its own offset and scale, every
image / chunk / column its own magnitude, weights differ per tap, channel and output row, and weight rows the kernel
must not use carry 1e4.  The helper-sensitivity tests at the end (no GPU) corrupt a correct result the way such a bug
would and require the comparison helpers to reject it.

Every test prints what it measured; the worst case per kernel on the MI355X is in DESIGN.md 5a "Per-kernel parity".
"""
import ctypes

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
EPS = 1e-6          # GroupNorm eps of the autoencoder (libs/autoencoder.py:31-32)
BF16_REL = 2.0 ** -8
NAN = float("nan")


# ---- comparison helpers (exercised without a GPU by the sensitivity tests below) -----------------------------------

def rel(a, b):
    a = torch.as_tensor(a).double()
    b = torch.as_tensor(b).double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def bf16_ulp(ref):
    return torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126))) - 7)


def ulp_err(out, ref, floor=2e-5):
    """max over elements of |out - ref| / max(one bf16 ulp at ref, floor); a NaN counts as infinite."""
    ref = ref.double()
    e = (out.double() - ref).abs() / bf16_ulp(ref).clamp_min(floor)
    return float(torch.nan_to_num(e, nan=float("inf")).max())


def assert_rel(out, ref, bound, what):
    r = rel(out, ref)
    print(f"{what}: rel-L2 = {r:.3e}")
    assert r < bound, (what, r)
    return r


def assert_one_ulp(out, ref, what):
    e = ulp_err(out, ref)
    print(f"{what}: max |d| / max(bf16 ulp, 2e-5) = {e:.3f}")
    assert e <= 1.0, (what, e)
    return e


def gn_reference(x, gamma, beta, swish, eps=EPS):
    """float64 GroupNorm(32) [+ swish] of NHWC x [B, P, C]: (y, mean [B, 32], rstd [B, 32], rms [B, 32])."""
    B, P, C = x.shape
    g = x.double().view(B, P, 32, C // 32)
    mean = g.mean((1, 3))
    msq = (g * g).mean((1, 3))
    var = ((g - mean[:, None, :, None]) ** 2).mean((1, 3))
    rstd = 1.0 / torch.sqrt(var + eps)
    u = ((g - mean[:, None, :, None]) * rstd[:, None, :, None]).reshape(B, P, C) * gamma.double() + beta.double()
    if swish:
        u = u * torch.sigmoid(u)
    return u, mean, rstd, msq.sqrt()


def assert_gn_stats(stats, mean, rstd, rms, what):
    """stats fp32 [B, 32, 2] = (mean, rstd) against float64."""
    s = stats.double()
    em = float(((s[..., 0] - mean).abs() / rms).max())
    er = float(((s[..., 1] - rstd).abs() / rstd).max())
    print(f"{what}: mean err / rms = {em:.3e}, rstd rel err = {er:.3e}")
    assert em <= 1e-6 and er <= 1e-5, (what, em, er)   # NaN fails both
    return em, er


def partials_reference(stored, B, gn_P):
    """float64 [B, gn_P / 256, 32, 3] = (sum, sum of squares, sum |x|) per 256-row chunk and group of stored [M, N]."""
    M, N = stored.shape
    v = stored.double().view(B, gn_P // 256, 256, 32, N // 32)
    return torch.stack([v.sum((2, 4)), (v * v).sum((2, 4)), v.abs().sum((2, 4))], -1)


def assert_gn_partials(part, stored, B, gn_P, what):
    """part: the fp64 partials [B * gn_P / 256 * 64] an epilogue wrote for the values `stored` it stored."""
    ref = partials_reference(stored, B, gn_P)
    p = part.view(B, gn_P // 256, 32, 2)
    assert not torch.isnan(p).any(), f"{what}: {int(torch.isnan(p).sum())} partial entries were never written"
    es = float(((p[..., 0] - ref[..., 0]).abs() / ref[..., 2]).max())
    eq = float(((p[..., 1] - ref[..., 1]).abs() / ref[..., 1]).max())
    print(f"{what}: max |d sum| / sum|x| = {es:.3e}, max |d sumsq| / sumsq = {eq:.3e}")
    assert es <= 1e-5 and eq <= 1e-5, (what, es, eq)
    return es, eq


def assert_softmax(p, ref, what):
    assert_one_ulp(p, ref, what)
    rs = float((p.double().sum(1) - 1.0).abs().max())
    print(f"{what}: max |row sum - 1| = {rs:.3e}")
    assert rs <= 2e-3, (what, rs)


# ---- inputs and float64 references -------------------------------------------------------------------------------

def gn_input(B, P, C, family, dev, seed):
    """x fp32 [B, P, C]: group g of image b is scale[b, g] * N(0, 1) + offset[b, g], every (b, g) its own scale in
    [0.5, 2) and offset; family 0: |mean| / std ~ 0.05, family 1: ~ 8 with alternating sign."""
    gen = torch.Generator(device=dev).manual_seed(seed)
    n = torch.randn(B, P, C, generator=gen, device=dev)
    idx = torch.arange(B * 32, device=dev).view(B, 32)
    scale = 0.5 + 1.5 * ((idx * 37) % 96).double() / 96.0
    r = (8.0 if family else 0.0) * (1 - 2 * (idx % 2)).double() + 0.05 * torch.sin(idx.double())
    x = n.double().view(B, P, 32, C // 32) * scale[:, None, :, None] + (scale * r)[:, None, :, None]
    return x.reshape(B, P, C).float()


def gn_affine(C, dev, seed, swish):
    gen = torch.Generator(device=dev).manual_seed(seed)
    gamma = 0.5 + torch.rand(C, generator=gen, device=dev)
    beta = torch.randn(C, generator=gen, device=dev) * 0.5
    if swish:   # u ~ -40 (swish ~ -1.7e-16) and u ~ -100 (2^(-u log2 e) overflows: exactly -0)
        gamma[5], beta[5] = 0.01, -40.0
        gamma[C - 3], beta[C - 3] = 0.01, -100.0
    return gamma, beta


def conv3x3_ref(x, w, up=0, stride=1):
    """float64 3x3 conv (pad 1) of NHWC x [B, h, w, C] with w [N, 3, 3, C] (ky, kx, ci) as nine shifted matmuls ->
    [B, H, W, N]; up = 1 convolves the nearest-x2 upsample."""
    x = x.double()
    if up:
        x = x.repeat_interleave(2, 1).repeat_interleave(2, 2)
    B, H, W, C = x.shape
    xp = torch.zeros(B, H + 2, W + 2, C, dtype=torch.float64, device=x.device)
    xp[:, 1:-1, 1:-1] = x
    out = torch.zeros(B, H, W, w.shape[0], dtype=torch.float64, device=x.device)
    for ky in range(3):
        for kx in range(3):
            out += xp[:, ky:ky + H, kx:kx + W] @ w[:, ky, kx].double().t()
    return out


def image_rows(B, H, W, C, dev, seed):
    """bf16 NHWC activations whose images, rows and channels all differ in magnitude."""
    gen = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(B, H, W, C, generator=gen, device=dev)
    x = x * (1.0 + 0.5 * torch.arange(B, device=dev).view(B, 1, 1, 1))
    x = x * (0.5 + torch.arange(H, device=dev).view(1, H, 1, 1) / H) + 0.25 * torch.sin(
        torch.arange(C, device=dev).float()).view(1, 1, 1, C)
    return x.bfloat16()


def conv_weight(N, C, dev, seed, rows=None):
    """bf16 [rows or N, 3, 3, C]: random (every tap / channel / row distinct), row o scaled by 1 + o / N; rows past N
    (padding the kernel must never use) hold 1e4."""
    gen = torch.Generator(device=dev).manual_seed(seed)
    w = torch.randn(N, 3, 3, C, generator=gen, device=dev) * (9 * C) ** -0.5
    w = w * (1.0 + torch.arange(N, device=dev).view(N, 1, 1, 1) / N)
    if rows and rows > N:
        w = torch.cat([w, torch.full((rows - N, 3, 3, C), 1.0e4, device=dev)])
    return w.bfloat16()


def softmax_scores(n, scale, dev):
    """fp32 scores [5, n] whose scaled values are: N(0, 1); 2 N(0, 1) + 7; a permuted ramp over [-60, 0]; N(0, 1) with
    the maximum in the last column; N(0, 1) - 20 with a peak in column 0."""
    gen = torch.Generator(device=dev).manual_seed(n)
    t = torch.randn(5, n, generator=gen, device=dev).double()
    t[1] = 2 * t[1] + 7
    t[2] = torch.linspace(-60.0, 0.0, n, device=dev, dtype=torch.float64)[torch.randperm(n, generator=gen, device=dev)]
    t[3, n - 1] = t[3].max() + 3
    t[4] -= 20
    t[4, 0] = t[4].max() + 5
    return (t / scale).float()


def softmax_ref(s, scale):
    return torch.softmax(s.double() * float(np.float32(scale)), dim=1)


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from panopticdiffusionmodels_amd import _lib
    _lib.load()
    return _lib


DEV = "cuda"


# ---- GroupNorm statistics and apply --------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("P", [64, 576, 4096])
@pytest.mark.parametrize("C", [64, 128, 192, 256, 512, 1024])
def test_groupnorm(lib, C, P, dtype):
    """gn_partial / gn_final / gn_apply.  C = 64: cpg 2, a channel octet straddles four groups; C = 192: cpg 6 and 48
    channel quads, which do not divide 256 (idle planes); P = 576 is ragged against the statistics chunk.  With swish
    two channels sit far negative: u ~ -40, whose swish -1.7e-16 is a normal bf16 number (so it is held to the float64
    value, not to 0: never NaN, never positive), and u ~ -100, where 2^(-u log2 e) overflows and the result must be
    exactly -0 or 0."""
    B = 3
    for family in (0, 1):
        x = gn_input(B, P, C, family, DEV, 1000 * C + P + family).to(dtype)
        for swish in (False, True):
            gamma, beta = gn_affine(C, DEV, C + P, swish)
            y, stats = lib.vae_groupnorm(x, gamma, beta, EPS, swish)
            ref, mean, rstd, rms = gn_reference(x, gamma, beta, swish)
            what = f"groupnorm C={C} P={P} {dtype} r={8 * family} swish={int(swish)}"
            assert_gn_stats(stats, mean, rstd, rms, what)
            assert_one_ulp(y, ref, what)
            if swish:
                assert not torch.isnan(y).any()
                assert float(y[..., 5].max()) <= 0.0                 # u ~ -40: -1.7e-16 (inside the 2e-5 floor above)
                assert float(y[..., C - 3].abs().max()) == 0.0       # u ~ -100: -0 or 0


@gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("P", [256, 1024, 4096])
@pytest.mark.parametrize("C", [64, 128, 256, 512, 1024])
def test_groupnorm_from_partials(lib, C, P, dtype):
    """Ready-made float64 partials in the GEMM epilogue's 256-pixel-chunk layout replace the statistics pass: the same
    (mean, rstd) and output, to the same bounds."""
    B = 3
    x = gn_input(B, P, C, 1, DEV, 77 * C + P).to(dtype)
    gamma, beta = gn_affine(C, DEV, C + P, True)
    part = partials_reference(x.reshape(B * P, C), B, P)[..., :2].contiguous()
    y, stats = lib.vae_groupnorm(x, gamma, beta, EPS, True, partials=part.view(-1))
    y0, stats0 = lib.vae_groupnorm(x, gamma, beta, EPS, True)
    ref, mean, rstd, rms = gn_reference(x, gamma, beta, True)
    what = f"groupnorm from partials C={C} P={P} {dtype}"
    assert_gn_stats(stats, mean, rstd, rms, what)
    assert_one_ulp(y, ref, what)
    assert_gn_stats(stats0, mean, rstd, rms, what + " (statistics pass)")
    d = float(((stats.double() - stats0.double()).abs() / torch.stack([rms, rstd], -1)).max())
    print(f"{what}: partials route vs statistics pass, max relative stats difference = {d:.3e}")
    assert d <= 1e-5


@gpu
def test_groupnorm_rejections(lib):
    g, b = torch.ones(1056, device=DEV), torch.zeros(1056, device=DEV)
    for B, P, C in [(1, 64, 48), (1, 64, 1056), (1, 64, 0)]:
        with pytest.raises(ValueError):
            lib.vae_groupnorm(torch.zeros(B, P, C, device=DEV), g, b)
    x = torch.zeros(1, 576, 64, device=DEV)
    with pytest.raises(ValueError):   # ready-made partials come in whole 256-pixel chunks
        lib.vae_groupnorm(x, g, b, partials=torch.zeros(3 * 64, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError):   # 16-byte loads
        lib.vae_groupnorm(torch.zeros(64 * 64 + 1, device=DEV)[1:].view(1, 64, 64), g, b)
    y = torch.empty(1, 576, 64, dtype=torch.bfloat16, device=DEV)
    st = torch.empty(1, 32, 2, device=DEV)
    small = torch.empty(63, dtype=torch.float64, device=DEV)
    assert lib.load().pdm_vae_groupnorm(lib.ptr(x), lib.PDM_F32, 1, 576, 64, lib.ptr(g), lib.ptr(b), EPS, 0,
                                        lib.ptr(small), 63, 0, lib.ptr(y), lib.ptr(st), None) == 1


# ---- the GroupNorm-partials epilogue of the GEMMs ----------------------------------------------------------------------

GUARD = 64


def nan_part(n):
    """n NaN doubles for the partials + GUARD more behind them that must stay NaN."""
    return torch.full((n + GUARD,), NAN, dtype=torch.float64, device=DEV)


def dense_problem(M, N, K, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    a = torch.randn(M, K, generator=gen, device=DEV)
    chunk = torch.arange(M, device=DEV) // 256
    a = (a * (0.5 + ((chunk * 5) % 16).float() / 8)[:, None] + 0.1).bfloat16()     # every 256-row chunk its own scale
    w = torch.randn(N, K, generator=gen, device=DEV) * K ** -0.5
    w = (w * (0.5 + ((torch.arange(N, device=DEV) // (N // 32) * 11) % 32).float() / 16)[:, None]).bfloat16()
    bias = ((torch.arange(N, device=DEV) * 7) % N).float() / N * 4 - 2             # every column its own offset
    r0 = torch.randn(M, N, generator=gen, device=DEV)
    return a, w, bias, r0, a.double() @ w.double().t() + bias.double()


def check_fused(lib, out, copy, part, fused, ref, B, gn_P, what, expect_fused):
    """The product is right either way; fused: every partial written and right, the guard untouched; not fused: the
    whole buffer still NaN."""
    n = lib.gn_part_elems(B, gn_P) if gn_P % 256 == 0 else part.numel() - GUARD
    if out.dtype == torch.float32:
        assert_rel(out, ref, 1e-5, what)
        if copy is not None:
            assert torch.equal(copy, out.bfloat16())
    else:
        assert_rel(out, ref, BF16_REL, what)
    assert fused in (0, 1)
    if expect_fused is not None:
        assert fused == int(expect_fused), (what, fused)
    if fused:
        assert_gn_partials(part[:n], out.float(), B, gn_P, what)
        assert torch.isnan(part[n:]).all(), f"{what}: wrote past the partials buffer"
    else:
        assert torch.isnan(part).all(), f"{what}: not fused, yet the partials buffer was written"


@gpu
@pytest.mark.parametrize("mode", ["f32", "f32acc", "f32copy", "f32acccopy"])
@pytest.mark.parametrize("gn_P", [256, 1024, 4096])
@pytest.mark.parametrize("N", [256, 512, 1024])
def test_gemm_gn_part_dense(lib, N, gn_P, mode):
    """The proj_out / downsample form: EPI_F32 (with / without accumulate and the bf16 copy), M = 4096, K = 256; cpg 8 /
    16 / 32, several column tiles once N > 256; 16 images of one chunk, 4 of 4, 1 of 16."""
    M, K = 4096, 256
    a, w, bias, r0, ref = dense_problem(M, N, K, N + gn_P)
    acc, cp = "acc" in mode, "copy" in mode
    out = r0.clone() if acc else torch.zeros(M, N, device=DEV)
    copy = torch.empty(M, N, dtype=torch.bfloat16, device=DEV) if cp else None
    part = nan_part(lib.gn_part_elems(M // gn_P, gn_P))
    out, fused = lib.gemm_gn(a, w, bias, lib.EPI_F32, part, gn_P, out=copy, out_f32=out, accumulate=acc)
    check_fused(lib, out, copy, part, fused, ref + r0.double() if acc else ref, M // gn_P, gn_P,
                f"gn_part dense N={N} gn_P={gn_P} {mode}", True)


@gpu
@pytest.mark.parametrize("case", ["M2048", "N192", "gn_P384", "M%gn_P", "algo1", "fusion_off"])
def test_gemm_gn_part_not_fused(lib, case):
    """Where the tile policy has no partials epilogue the entry says so, leaves gn_part alone and still computes the
    product."""
    M, N, K, gn_P = 4096, 256, 256, 256
    if case == "M2048":
        M = 2048
    elif case == "N192":
        N = 192
    elif case == "gn_P384":
        gn_P = 384
    elif case == "M%gn_P":
        M, gn_P = 4096 + 256, 1024
    a, w, bias, _, ref = dense_problem(M, N, K, len(case))
    part = nan_part(M // 256 * 64)
    L = lib.load()
    try:
        if case == "algo1":
            lib.check(L.pdm_set_gemm_algo(1))
        if case == "fusion_off":
            lib.check(L.pdm_decoder_set_gn_fusion(0))
        out, fused = lib.gemm_gn(a, w, bias, lib.EPI_F32, part, gn_P)
    finally:
        L.pdm_set_gemm_algo(0)
        L.pdm_decoder_set_gn_fusion(1)
    check_fused(lib, out, None, part, fused, ref, M // gn_P, gn_P, f"gn_part not fused: {case}", False)


@gpu
@pytest.mark.parametrize("M,N,K,gn_P,epi", [
    (4096, 256, 64, 256, "f32"), (3840, 256, 64, 256, "f32"), (4096, 256, 64, 256, "bf16"), (8192, 2048, 64, 512, "f32"),
    (8192, 96, 64, 256, "f32"), (65536, 128, 64, 256, "f32"), (32768, 128, 64, 256, "f32"), (65536, 128, 64, 65536, "f32"),
    (4096, 288, 64, 256, "f32"), (4352, 512, 64, 256, "f32"), (4096, 512, 576, 4096, "f32")])
def test_gemm_gn_part_policy_mirror(lib, M, N, K, gn_P, epi):
    """gemm_gn_fusable mirrors gemm_launch's tile choice; the two must not drift: whatever the entry reports, it is
    true -- fused means every partial was written (and is right), not fused means none was."""
    a, w, bias, _, ref = dense_problem(M, N, K, M + N + gn_P)
    part = nan_part(lib.gn_part_elems(M // gn_P, gn_P))
    e = lib.EPI_F32 if epi == "f32" else lib.EPI_BF16
    pl = lib.gemm_plan(lib.gemm_shape_args(M, N, K, e), e, gn_P=gn_P)
    out, fused = lib.gemm_gn(a, w, bias, e, part, gn_P)
    # the entry's answer is the plan's: the epilogue of the planned kernel writes the partials, and their shape rule
    shape_ok = gn_P % 256 == 0 and M % gn_P == 0 and N % 32 == 0 and N // 32 in (4, 8, 16, 32)
    assert pl.error is None and bool(fused) == pl.gn_fusable == (pl.writes_gn and shape_ok), (fused, pl)
    check_fused(lib, out, None, part, fused, ref, M // gn_P, gn_P, f"gn_part policy M={M} N={N} gn_P={gn_P} {epi}", None)
    print(f"gn_part policy M={M} N={N} gn_P={gn_P} {epi}: fused = {fused}")


def conv_problem(B, h, Cin, N, up, seed):
    x = image_rows(B, h, h, Cin, DEV, seed)
    w = conv_weight(N, Cin, DEV, seed + 1)
    bias = ((torch.arange(N, device=DEV) * 7) % N).float() / N * 4 - 2
    ref = conv3x3_ref(x, w, up).view(-1, N) + bias.double()
    return x, w.permute(0, 3, 1, 2).contiguous(), bias, ref   # w back in the torch layout gemm_conv3x3 takes


def run_conv_gn(lib, x, w, bias, ref, mode, up, what):
    B, H = x.shape[0], x.shape[1] << up
    M, N = B * H * H, w.shape[0]
    part = nan_part(lib.gn_part_elems(B, H * H))
    copy = None
    e = lib.EPI_BF16 if mode == "bf16" else lib.EPI_F32
    Cin = x.shape[3]
    pl = lib.gemm_plan(lib.gemm_shape_args(M, N, 9 * Cin, e, conv_C=Cin, copy=mode == "f32copy", accumulate=mode == "f32acc"),
                       e, conv=(H, H, Cin, up), gn_P=H * H)
    if mode == "bf16":      # conv1: the partials of the ROUNDED values
        out, fused = lib.gemm_conv3x3_gn(x, w, bias, lib.EPI_BF16, part, up=up)
    elif mode == "f32acc":  # conv2
        r0 = torch.randn(M, N, generator=torch.Generator(device=DEV).manual_seed(M), device=DEV)
        ref = ref + r0.double()
        out, fused = lib.gemm_conv3x3_gn(x, w, bias, lib.EPI_F32, part, up=up, out_f32=r0.clone(), accumulate=True)
    else:                   # the upsample conv: fp32 with the bf16 copy
        copy = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
        out, fused = lib.gemm_conv3x3_gn(x, w, bias, lib.EPI_F32, part, up=up, out=copy)
    assert pl.error is None and bool(fused) == pl.writes_gn == pl.gn_fusable, (what, fused, pl)
    check_fused(lib, out, copy, part, fused, ref, B, H * H, what, True)


@gpu
@pytest.mark.parametrize("mode,up", [("bf16", 0), ("f32acc", 0), ("f32copy", 1)])
def test_gemm_gn_part_conv(lib, mode, up):
    """The conv forms at 4 x 32^2, Cin 64 -> N 256 (256-row tiles of whole images)."""
    x, w, bias, ref = conv_problem(4, 32 >> up, 64, 256, up, 7 + up)
    run_conv_gn(lib, x, w, bias, ref, mode, up, f"gn_part conv {mode} up={up}")


@gpu
@pytest.mark.parametrize("mode", ["bf16", "f32acc"])
@pytest.mark.parametrize("B,h", [(1, 256), (16, 64), (256, 16)])
def test_gemm_gn_part_conv_tall_tile(lib, B, h, mode):
    """N = 128 (cpg 4: two slots per thread) on the 512-row tile, M = 65536: one image; 16 x 64^2 (a tile holds two
    chunks of one image); 256 x 16^2 (a tile holds two images)."""
    x, w, bias, ref = conv_problem(B, h, 64, 128, 0, B + h)
    run_conv_gn(lib, x, w, bias, ref, mode, 0, f"gn_part conv tall tile {B} x {h}^2 {mode}")


# ---- softmax rows, transpose --------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("n", [64, 576, 1024, 4096])
def test_softmax_rows(lib, n):
    scale = 512 ** -0.5
    s = softmax_scores(n, scale, DEV)
    guard = torch.full((5 * n + 4096,), 7.0, dtype=torch.bfloat16, device=DEV)   # rows must end where they end
    p = lib.vae_softmax_rows(s, scale)
    assert_softmax(p, softmax_ref(s, scale), f"softmax n={n}")
    L = lib.load()
    lib.check(L.pdm_vae_softmax_rows(lib.ptr(s), lib.ptr(guard), 5, n, scale, lib.stream_ptr(s.device)))
    assert torch.equal(guard[:5 * n].view(5, n), p) and bool((guard[5 * n:] == 7.0).all())


@gpu
def test_softmax_rows_rejects_long_rows(lib):
    with pytest.raises(ValueError, match="4096"):
        lib.vae_softmax_rows(torch.zeros(2, 4097, device=DEV), 1.0)
    with pytest.raises(ValueError):
        lib.vae_softmax_rows(torch.zeros(2, 5184, device=DEV), 1.0)


@gpu
@pytest.mark.parametrize("n,C", [(64, 128), (576, 512)])
def test_transpose(lib, n, C):
    B, ld, col0 = 2, 3 * C, 2 * C
    gen = torch.Generator(device=DEV).manual_seed(n)
    src = torch.full((B, n, ld), 0x7FC1, dtype=torch.int16, device=DEV)            # sentinel bit pattern
    src[:, :, col0:] = torch.randint(0, 0x7F80, (B, n, C), generator=gen, device=DEV).to(torch.int16)
    out = lib.vae_transpose(src.view(torch.bfloat16), col0, C).view(torch.int16)
    assert torch.equal(out, src[:, :, col0:].transpose(1, 2).contiguous())
    assert not bool((out == 0x7FC1).any())
    with pytest.raises(ValueError):
        lib.vae_transpose(src.view(torch.bfloat16)[:, :48].contiguous(), col0, C)   # n % 32
    with pytest.raises(ValueError):
        lib.vae_transpose(src.view(torch.bfloat16), col0, C - 16)                    # C % 32
    with pytest.raises(ValueError):
        lib.vae_transpose(src.view(torch.bfloat16), col0 + 32, C)                    # past the row


# ---- decoder conv_in / conv_out ---------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("Cout", [128, 512])
@pytest.mark.parametrize("h", [8, 24, 64])
def test_dec_conv_in(lib, h, Cout):
    B, scale = 2, 0.18215
    gen = torch.Generator(device=DEV).manual_seed(h + Cout)
    z = torch.randn(B, 4, h, h, generator=gen, device=DEV) * torch.tensor([1.0, 2.5], device=DEV).view(2, 1, 1, 1)
    z = z * (0.5 + torch.arange(h, device=DEV).view(1, 1, h, 1) / h)
    pq_w = torch.randn(4, 4, generator=gen, device=DEV)
    pq_b = torch.randn(4, generator=gen, device=DEV)
    w = torch.randn(Cout, 4, 3, 3, generator=gen, device=DEV) / 6
    bias = torch.randn(Cout, generator=gen, device=DEV)
    out = lib.vae_dec_conv_in(z, scale, pq_w, pq_b, w, bias)
    zz = torch.einsum("oc,bchw->bhwo", pq_w.double(), z.double() / float(np.float32(scale))) + pq_b.double()
    ref = conv3x3_ref(zz, w.permute(0, 2, 3, 1)) + bias.double()
    assert_rel(out, ref, 1e-5, f"dec conv_in h={h} Cout={Cout}")


@gpu
def test_dec_conv_in_rejects_wide_latents(lib):
    z = torch.zeros(1, 4, 8, 72, device=DEV)
    w = torch.zeros(64, 4, 3, 3, device=DEV)
    with pytest.raises(ValueError, match="64"):
        lib.vae_dec_conv_in(z, 1.0, torch.zeros(4, 4, device=DEV), torch.zeros(4, device=DEV), w,
                            torch.zeros(64, device=DEV))


def conv_out_problem(B, H, C, dev, rows=4, N=3):
    g = image_rows(B, H, H, C, dev, H + C)
    w = conv_weight(N, C, dev, H + C + 1, rows=rows)
    bias = torch.tensor([0.3, -0.7, 1.1, 1.0e4, 5.0, -6.0, 7.0, -8.0], device=dev)[:rows].contiguous()
    ref = (conv3x3_ref(g, w[:N]) + bias[:N].double()).permute(0, 3, 1, 2)
    return g, w, bias, ref


@gpu
@pytest.mark.parametrize("B,H,C,force_valu", [
    (2, 64, 64, False), (2, 64, 128, False), (2, 128, 64, False), (2, 128, 128, False),
    (2, 64, 64, True), (2, 64, 128, True), (2, 128, 64, True), (2, 128, 128, True),
    (2, 48, 64, False), (3, 24, 192, False)])
def test_dec_conv_out(lib, B, H, C, force_valu):
    """The MFMA kernel (C 64 / 128; 128^2 takes two 64-pixel segments per row and restages LDS) and the VALU kernel
    (forced at the same shapes, and chosen at 48^2 and C = 192).  The weight's padding row and its bias hold 1e4."""
    g, w, bias, ref = conv_out_problem(B, H, C, DEV)
    img = lib.vae_dec_conv_out(g, w, bias, 3, force_valu)
    assert_rel(img, ref, 1e-5, f"dec conv_out {B} x {H}^2 C={C} {'VALU' if force_valu or H % 64 or C > 128 else 'MFMA'}")
    assert float(img.abs().max()) < 100.0


@gpu
def test_dec_conv_out_rejections(lib):
    g, w, bias, _ = conv_out_problem(1, 8, 64, DEV)
    with pytest.raises(ValueError):
        lib.vae_dec_conv_out(g, w, bias, 5)
    with pytest.raises(ValueError):
        lib.vae_dec_conv_out(g[..., :60].contiguous(), w, bias, 3)       # C % 8
    with pytest.raises(ValueError):   # 9 * C * 16 bytes of fp32 weights do not fit the VALU kernel's LDS
        lib.vae_dec_conv_out(torch.zeros(1, 8, 8, 512, dtype=torch.bfloat16, device=DEV),
                             torch.zeros(4, 3, 3, 512, dtype=torch.bfloat16, device=DEV), bias, 3)


# ---- encoder conv_in / downsample gather / tail ----------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("C", [64, 128, 320])
@pytest.mark.parametrize("H,W", [(16, 24), (24, 40), (8, 512)])
def test_enc_conv_in(lib, H, W, C):
    """W not a multiple of 16, and the limit 512; H != W; C = 320 runs the second blockIdx.z slice with 64 channels.
    The kernel rounds image and weight to bf16: so does the reference."""
    B = 2
    gen = torch.Generator(device=DEV).manual_seed(H + W + C)
    img = torch.rand(B, 3, H, W, generator=gen, device=DEV) * 2 - 1
    img = img * torch.tensor([1.0, 0.5], device=DEV).view(2, 1, 1, 1) + 0.1 * torch.arange(3, device=DEV).view(1, 3, 1, 1)
    w = torch.randn(C, 3, 3, 3, generator=gen, device=DEV) * (1 + torch.arange(C, device=DEV).view(C, 1, 1, 1) / C) / 5
    bias = torch.randn(C, generator=gen, device=DEV)
    out = lib.vae_enc_conv_in(img, w, bias)
    ref = conv3x3_ref(img.bfloat16().permute(0, 2, 3, 1), w.bfloat16().permute(0, 2, 3, 1)) + bias.double()
    assert_rel(out, ref, 1e-5, f"enc conv_in {H} x {W} C={C}")


@gpu
def test_enc_conv_in_rejections(lib):
    b = torch.zeros(64, device=DEV)
    with pytest.raises(ValueError):
        lib.vae_enc_conv_in(torch.zeros(1, 3, 8, 520, device=DEV), torch.zeros(64, 3, 3, 3, device=DEV), b)
    with pytest.raises(ValueError):
        lib.vae_enc_conv_in(torch.zeros(1, 3, 8, 16, device=DEV), torch.zeros(40, 3, 3, 3, device=DEV), b)


@gpu
@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("H,W", [(16, 16), (48, 48), (16, 24)])
def test_down_gather(lib, H, W, C):
    B = 2
    gen = torch.Generator(device=DEV).manual_seed(H * W + C)
    x = torch.randn(B, H, W, C, generator=gen, device=DEV)
    x = x + torch.where(x >= 0, 0.5, -0.5)        # no zeros in the data: the padding's zeros are the only ones
    A = lib.vae_down_gather(x)
    xp = torch.zeros(B, H + 1, W + 1, C, device=DEV)
    xp[:, :H, :W] = x
    ref = torch.stack([xp[:, ky:ky + H:2, kx:kx + W:2] for ky in range(3) for kx in range(3)], 3)   # [B, Ho, Wo, 9, C]
    assert torch.equal(A, ref.reshape(B * (H // 2) * (W // 2), 9 * C).bfloat16())
    v = A.view(B, H // 2, W // 2, 3, 3, C)
    assert bool((v[:, -1, :, 2] == 0).all()) and bool((v[:, :, -1, :, 2] == 0).all())   # row H, column W
    assert int((v == 0).sum()) == B * C * (3 * (W // 2) + 3 * (H // 2) - 1)
    with pytest.raises(ValueError):
        lib.vae_down_gather(x[:, :H - 1].contiguous())


@gpu
@pytest.mark.parametrize("B,H,W", [(3, 5, 7), (2, 8, 8)])
@pytest.mark.parametrize("C", [64, 128, 512])
def test_enc_tail(lib, C, B, H, W):
    """conv_out + quant_conv.  C = 64: 18 k-steps dealt 5 / 5 / 4 / 4 to the waves; 3 x 5 x 7 = 105 pixels: 16-pixel
    blocks straddle rows and images and the last one is ragged."""
    gen = torch.Generator(device=DEV).manual_seed(C + H)
    g = image_rows(B, H, W, C, DEV, C + H)
    w = conv_weight(8, C, DEV, C + H + 1)
    cbias = torch.randn(8, generator=gen, device=DEV)
    qw = torch.randn(8, 8, generator=gen, device=DEV)
    qb = torch.randn(8, generator=gen, device=DEV)
    m = lib.vae_enc_tail(g, w, cbias, qw, qb)
    h = conv3x3_ref(g, w) + cbias.double()
    ref = (h @ qw.double().t() + qb.double()).permute(0, 3, 1, 2)
    assert_rel(m, ref, 1e-5, f"enc tail {B} x {H} x {W} C={C}")
    with pytest.raises(ValueError):
        lib.vae_enc_tail(g[..., :48].contiguous(), w[..., :48].contiguous(), cbias, qw, qb)


# ---- the encoder's size limit ------------------------------------------------------------------------------------------

def _enc_cfg(lib, latent):
    cfg = lib.PdmEncoderCfg()
    cfg.ch, cfg.num_levels, cfg.num_res_blocks = 64, 2, 1
    cfg.ch_mult[0], cfg.ch_mult[1] = 1, 2
    cfg.in_channels, cfg.z_channels, cfg.double_z, cfg.latent_size = 3, 4, 1, latent
    return cfg


def test_encoder_create_rejects_latents_past_the_softmax():
    """A two-level encoder at latent 72 (image side 144 <= 512) has 5184 attention tokens; the row softmax takes 4096.
    Create is pure host code."""
    from panopticdiffusionmodels_amd import _lib
    L = _lib.load()
    h = ctypes.c_void_p()
    with pytest.raises(ValueError, match="4096"):
        _lib.check(L.pdm_encoder_create(ctypes.byref(_enc_cfg(_lib, 72)), ctypes.byref(h)))
    _lib.check(L.pdm_encoder_create(ctypes.byref(_enc_cfg(_lib, 64)), ctypes.byref(h)))
    L.pdm_encoder_destroy(h)


def _two_level_ae(seed):
    from panopticdiffusionmodels_amd import weights as W
    from panopticdiffusionmodels_amd.libs.autoencoder import FrozenAutoencoderKL
    sd = W.make_state_dict(W.decoder_spec(ch=64, ch_mult=(1, 2), num_res_blocks=1), seed=seed, init="random")
    esd = W.encoder_state_dict(seed=seed, init="random", ch=64, ch_mult=(1, 2), num_res_blocks=1)
    sd.update(esd)
    dd = dict(W.DECODER_DDCONFIG, ch=64, ch_mult=[1, 2], num_res_blocks=1)
    return FrozenAutoencoderKL(dd, 4, state_dict=sd), esd


def test_oracle_encode_matches_reference_fixture():
    """oracle.autoencoder_ref.encode_moments (the reference of the size-limit test below) reproduces the reference
    encoder's own fp32 moments of the enc64 fixture (tests/golden/encoder_golden.npz)."""
    import os
    from oracle import autoencoder_ref
    from panopticdiffusionmodels_amd import weights as W
    fx = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encoder_golden.npz"))
    esd = W.encoder_state_dict(seed=31, init="random", ch=64, ch_mult=(1, 2), num_res_blocks=1)
    x = torch.rand(3, 3, 48, 48, generator=torch.Generator().manual_seed(1031)) * 2.0 - 1.0
    with torch.no_grad():
        m = autoencoder_ref.encode_moments(esd, x, ch_mult=(1, 2), num_res_blocks=1)
    assert rel(m, fx["enc64/moments"]) < 1e-5


@gpu
def test_encoder_two_level_size_limit(lib):
    """The two-level model encodes up to 128^2 (latent 64, 4096 attention tokens: against the fp32 oracle within the
    encoder's 2e-2) and refuses 144^2."""
    from oracle import autoencoder_ref
    ae, esd = _two_level_ae(52)
    ae = ae.to(DEV)
    with pytest.raises(ValueError, match="4096"):
        ae.encode_moments(torch.zeros(1, 3, 144, 144, device=DEV))
    x = torch.rand(1, 3, 128, 128, generator=torch.Generator().manual_seed(1052)) * 2.0 - 1.0
    m = ae.encode_moments(x.to(DEV)).cpu()
    with torch.no_grad():
        ref = autoencoder_ref.encode_moments(esd, x, ch_mult=(1, 2), num_res_blocks=1)
    r = rel(m, ref)
    print(f"two-level encoder at 128^2 (hw = 4096): rel-L2(moments) = {r:.3e}")
    assert m.shape == (1, 8, 64, 64) and r < 2e-2


# ---- helper sensitivity (no GPU): each comparison rejects the bug it is there for ------------------------------------

def test_helper_rejects_swapped_group_statistics():
    B, P, C = 2, 64, 64
    x = gn_input(B, P, C, 1, "cpu", 1)
    gamma, beta = gn_affine(C, "cpu", 2, False)
    _, mean, rstd, rms = gn_reference(x, gamma, beta, False)
    stats = torch.stack([mean, rstd], -1).float()
    assert_gn_stats(stats, mean, rstd, rms, "correct statistics")
    bad = stats.clone()
    bad[1, [3, 5]] = stats[1, [5, 3]]          # two groups of one image swapped (same sign of the mean)
    with pytest.raises(AssertionError):
        assert_gn_stats(bad, mean, rstd, rms, "swapped groups")
    bad = stats.clone()
    bad[0], bad[1] = stats[1], stats[0]        # the other image's statistics
    with pytest.raises(AssertionError):
        assert_gn_stats(bad, mean, rstd, rms, "swapped images")
    # ... and the apply check sees statistics taken from the neighbouring group
    ref, _, _, _ = gn_reference(x, gamma, beta, True)
    assert_one_ulp(ref.bfloat16(), ref, "correct output")
    m2, r2 = mean.clone(), rstd.clone()
    m2[1, [3, 5]], r2[1, [3, 5]] = mean[1, [5, 3]], rstd[1, [5, 3]]
    u = ((x.double().view(B, P, 32, 2) - m2[:, None, :, None]) * r2[:, None, :, None]).reshape(B, P, C)
    u = u * gamma.double() + beta.double()
    with pytest.raises(AssertionError):
        assert_one_ulp((u * torch.sigmoid(u)).bfloat16(), ref, "applied with the neighbouring group's statistics")


def test_helper_rejects_dropped_or_misplaced_chunk_partial():
    B, gn_P, N = 2, 512, 128
    gen = torch.Generator().manual_seed(3)
    stored = torch.randn(B * gn_P, N, generator=gen) * (1 + torch.arange(B * gn_P) // 256)[:, None] + 0.3
    part = partials_reference(stored, B, gn_P)[..., :2].contiguous().view(-1)
    assert_gn_partials(part, stored, B, gn_P, "correct partials")
    bad = part.clone()
    bad.view(B, 2, 32, 2)[1, 0] = NAN                      # one chunk never written
    with pytest.raises(AssertionError, match="never written"):
        assert_gn_partials(bad, stored, B, gn_P, "dropped chunk")
    bad = part.clone()
    bad.view(B, 2, 32, 2)[1, 0] = part.view(B, 2, 32, 2)[1, 1]   # a chunk's partial written to its neighbour's slot
    with pytest.raises(AssertionError):
        assert_gn_partials(bad, stored, B, gn_P, "misplaced chunk")
    bad = part.clone()
    bad.view(B, 2, 32, 2)[0, 1, 7, 1] *= 1 + 1e-4          # one entry off: every entry is compared, not a norm
    with pytest.raises(AssertionError):
        assert_gn_partials(bad, stored, B, gn_P, "one entry off")


def test_helper_rejects_shifted_softmax_row():
    scale = 512 ** -0.5
    s = softmax_scores(576, scale, "cpu")
    ref = softmax_ref(s, scale)
    p = ref.bfloat16()
    assert_softmax(p, ref, "correct softmax")
    for row in range(5):
        bad = p.clone()
        bad[row] = torch.roll(p[row], 1)
        with pytest.raises(AssertionError):
            assert_softmax(bad, ref, f"row {row} shifted by a column")
    bad = p.clone()
    bad[0, 256:] = 0                                        # a row short by a block
    with pytest.raises(AssertionError):
        assert_softmax(bad, ref, "row short by a block")


def test_helper_rejects_duplicated_conv_out_row():
    g, w, bias, ref = conv_out_problem(2, 16, 64, "cpu")
    img = ref.float()
    assert_rel(img, ref, 1e-5, "correct conv_out")
    bad = img.clone()
    bad[1, :, 7] = img[1, :, 6]                             # one image's row duplicated from its neighbour
    with pytest.raises(AssertionError):
        assert_rel(bad, ref, 1e-5, "duplicated row")
    bad = img.clone()
    bad[1, :, :, 0] = img[1, :, :, 1]                       # a wrong halo column
    with pytest.raises(AssertionError):
        assert_rel(bad, ref, 1e-5, "wrong first column")
    # the padding row's 1e4 weights would swamp the output if a kernel used them
    with pytest.raises(AssertionError):
        assert_rel((conv3x3_ref(g, w)[..., 1:4] + bias[1:4].double()).permute(0, 3, 1, 2), ref, 1e-5, "rows shifted")
