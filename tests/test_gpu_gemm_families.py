"""The smallest shape that reaches each GEMM kernel family under the automatic policy: the output against float64 on the
same operands (tolerances of the neighbouring tests: tests/test_gpu_kernels.py, tests/test_gpu_fp8.py), and the family
asserted through pdm_gemm_plan -- so a policy change that reroutes one of these shapes fails here by name."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def rel(a, b):
    return float((a.double() - b).norm() / b.norm().clamp_min(1e-30))


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from panopticdiffusionmodels_amd import _lib
    _lib.load()
    return _lib


def operands(M, N, K, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    a = torch.randn(M, K, device="cuda", generator=g).bfloat16()
    w = (torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).bfloat16()
    return a, w, torch.randn(N, device="cuda", generator=g)


def planned(lib, g, epi, family, **kw):
    pl = lib.gemm_plan(g, epi, **kw)
    print(f"gemm plan: {pl.family} epi {pl.epi} grid {pl.grid_x} x {pl.grid_y}")
    assert pl.error is None and pl.family == family and not pl.split_m1, pl
    return pl


def test_persistent_8s_gelu(lib):
    M, N, K = 4133, 1000, 1024   # ragged rows, a 232-column last tile
    a, w, bias = operands(M, N, K, 1)
    out = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
    planned(lib, lib._gemm_args(a, w, bias, out=out), lib.EPI_GELU, "8s")
    lib.gemm_ex(lib.EPI_GELU, a, w, bias, out=out)
    assert rel(out, F.gelu(a.double() @ w.double().t() + bias.double())) < 1e-2


def test_128_tile(lib):
    M, N, K = 515, 768, 2048     # below 4096 rows
    a, w, bias = operands(M, N, K, 2)
    out = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
    planned(lib, lib._gemm_args(a, w, bias, out=out), lib.EPI_BF16, "128")
    lib.gemm_ex(lib.EPI_BF16, a, w, bias, out=out)
    assert rel(out, a.double() @ w.double().t() + bias.double()) < 1e-2


def test_8d_conv(lib):
    B, h, Cin, N = 4, 32, 64, 256
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(B, h, h, Cin, device="cuda", generator=g).bfloat16()
    w = (torch.randn(N, Cin, 3, 3, device="cuda", generator=g) * (9 * Cin) ** -0.5).bfloat16()
    bias = torch.randn(N, device="cuda", generator=g)
    pl = planned(lib, lib.gemm_shape_args(B * h * h, N, 9 * Cin, lib.EPI_F32, conv_C=Cin), lib.EPI_F32, "8d",
                 conv=(h, h, Cin, 0))
    assert pl.conv == 1 and pl.sched == 2
    out = lib.gemm_conv3x3(x, w, bias, lib.EPI_F32)
    ref = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), bias.double(), padding=1).permute(0, 2, 3, 1).reshape(-1, N)
    assert rel(out, ref) < 2e-3


def test_8t_tall(lib):
    M, N, K = 65536, 128, 64     # one K-tile: the shortest main loop
    a, w, bias = operands(M, N, K, 4)
    out = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
    planned(lib, lib._gemm_args(a, w, bias, out=out), lib.EPI_BF16, "8t")
    lib.gemm_ex(lib.EPI_BF16, a, w, bias, out=out)
    assert rel(out, a.double() @ w.double().t() + bias.double()) < 1e-2


@pytest.mark.parametrize("M,family", [(4128, "8s_mx"), (2064, "mx")])
def test_mxfp8_operands(lib, M, family):
    N, K = 1024, 1024            # 16 / 8 sequences of 258 tokens: at and below the persistent form's 4096 rows
    g = torch.Generator(device="cuda").manual_seed(M)
    a = torch.randn(M, K, device="cuda", generator=g) * 2
    w = torch.randn(N, K, device="cuda", generator=g) * K ** -0.5
    bias = torch.randn(N, device="cuda", generator=g)
    (qa, sa), (qw, sw) = lib.mx_quantize(a), lib.mx_quantize(w)
    out = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
    pl = planned(lib, lib._gemm_args(qa, qw, bias, sa, sw, out), lib.EPI_BF16, family)
    assert pl.fp8 == 1
    lib.gemm_ex(lib.EPI_BF16, qa, qw, bias, sa, sw, out=out)
    ref = lib.mx_dequantize(qa, sa).double() @ lib.mx_dequantize(qw, sw).double().t() + bias.double()
    assert rel(out, ref) < 5e-3


def test_grouped_pair_8g(lib):
    N, K = 512, 512
    pair = []
    for M in (4133, 4200):
        a, w, bias = operands(M, N, K, M)
        res = torch.randn(M, N, device="cuda", generator=torch.Generator(device="cuda").manual_seed(M + 1)).bfloat16()
        pair.append(dict(a=a, w=w, bias=bias, out=torch.empty(M, N, device="cuda", dtype=torch.bfloat16), res_in=res,
                         accumulate=True, stats_out=torch.empty(M, 2, 2, device="cuda")))
    pl = planned(lib, lib._gemm_args(**pair[0]), lib.EPI_RES, "8g", second=lib._gemm_args(**pair[1]))
    assert pl.grouped and (pl.nt0, pl.ntiles) == (34, 68)
    lib.gemm_pair(lib.EPI_RES, *pair)
    for kw in pair:
        ref = kw["a"].double() @ kw["w"].double().t() + kw["bias"].double() + kw["res_in"].double()
        assert rel(kw["out"], ref) < 4e-3    # one bf16 rounding of the fp32 sum
