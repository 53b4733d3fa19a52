"""sha256 of the GEMM outputs' bits at the shapes that matter: one shape per kernel family under the automatic policy
(tests/test_gpu_gemm_families.py), the block Linears of the shipped configs at the bench's per-lane row counts (bf16,
and MXFP8 for U-ViT-H/4), and the decoder's conv3x3 shapes at latent 32.  Run from the repository root, once per build,
and compare the BITS lines:
    python tools/gemm_hash.py > new.log; PDM_LIB_PATH=path/to/other/libpdm.so python tools/gemm_hash.py > old.log
The PLAN line before each BITS line names the kernel family (pdm_gemm_plan; "-" from a library without it).
(profiles/gemm_plan/gemm_hash_*.log: the dispatcher refactoring against its parent)."""
import hashlib
import sys

import torch

sys.path.insert(0, ".")
from panopticdiffusionmodels_amd import _lib

HAS_PLAN = hasattr(_lib.load(), "pdm_gemm_plan")
BF = torch.bfloat16


def bits(*ts):
    h = hashlib.sha256()
    for t in ts:
        h.update(t.contiguous().view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()[:24]


def report(name, epi, kw, outs, second=None, conv=None):
    fam = "-"
    if HAS_PLAN:
        g = kw if isinstance(kw, _lib.PdmGemmArgs) else _lib._gemm_args(**kw)
        pl = _lib.gemm_plan(g, epi, second=_lib._gemm_args(**second) if second else None, conv=conv)
        fam = f"{pl.family} epi {pl.epi} conv {pl.conv} sched {pl.sched} mxo {pl.mxo} fp8 {pl.fp8} dual {pl.dual}"
    torch.cuda.synchronize()
    print(f"PLAN {name}: {fam}")
    print(f"BITS {name} {bits(*outs)}", flush=True)


def rnd(g, *shape, scale=1.0):
    return torch.randn(*shape, device="cuda", generator=g) * scale


def linear(name, M, N, K, kind, g, fp8=False):
    """kind: qkv (LayerNorm consumer, bf16), fc1 (consumer, GELU; fp8: the MXFP8 copy as its only output), proj / fc2
    (bf16 residual in place + LayerNorm partials), skip (the same over a split-K operand)."""
    w = rnd(g, N, K, scale=K ** -0.5)
    bias = rnd(g, N)
    if kind in ("qkv", "fc1"):
        epi = _lib.EPI_BF16 if kind == "qkv" else _lib.EPI_GELU
        x = rnd(g, M, K, scale=1.3) + 0.2
        if fp8 and kind == "qkv":   # MXFP8 operands, plain bf16 epilogue
            (qa, sa), (qw, sw) = _lib.mx_quantize(x), _lib.mx_quantize(w)
            kw = dict(a=qa, w=qw, bias=bias, a_scale=sa, w_scale=sw, out=torch.empty(M, N, device="cuda", dtype=BF))
            _lib.gemm_ex(epi, **kw)
            return report(name, epi, kw, [kw["out"]])
        xb, st = _lib.rowstats(x)
        wb = w.to(BF)
        kw = dict(a=xb, w=wb, bias=bias, ln_stats=st, ln_colsum=wb.float().sum(1))
        if fp8:
            kw.update(out_fp8=torch.empty(M, N, device="cuda", dtype=torch.float8_e4m3fn),
                      out_scale=torch.zeros((N + 127) // 128, M, device="cuda", dtype=torch.int32))
            outs = [kw["out_fp8"], kw["out_scale"]]
        else:
            kw["out"] = torch.empty(M, N, device="cuda", dtype=BF)
            outs = [kw["out"]]
        _lib.gemm_ex(epi, **kw)
        return report(name, epi, kw, outs)
    kk = K // 2 if kind == "skip" else K
    a = rnd(g, M, kk)
    out = rnd(g, M, N, scale=2.0).to(BF)
    kw = dict(bias=bias, out=out, res_in=out, accumulate=True, stats_out=torch.empty(M, (N + 255) // 256, 2, device="cuda"))
    if fp8:
        (qa, sa), (qw, sw) = _lib.mx_quantize(a), _lib.mx_quantize(w)
        kw.update(a=qa, w=qw, a_scale=sa, w_scale=sw)
    else:
        kw.update(a=a.to(BF), w=w.to(BF))
        if kind == "skip":
            kw["a2"] = rnd(g, M, kk).to(BF)
    _lib.gemm_ex(_lib.EPI_RES, **kw)
    report(name, _lib.EPI_RES, kw, [kw["out"], kw["stats_out"]])


def main():
    g = torch.Generator(device="cuda").manual_seed(11)
    # ---- one shape per family (tests/test_gpu_gemm_families.py)
    for name, M, N, K, epi in (("8s 4133x1000x1024 gelu", 4133, 1000, 1024, _lib.EPI_GELU),
                               ("128 515x768x2048", 515, 768, 2048, _lib.EPI_BF16),
                               ("8t 65536x128x64", 65536, 128, 64, _lib.EPI_BF16)):
        kw = dict(a=rnd(g, M, K).to(BF), w=rnd(g, N, K, scale=K ** -0.5).to(BF), bias=rnd(g, N),
                  out=torch.empty(M, N, device="cuda", dtype=BF))
        _lib.gemm_ex(epi, **kw)
        report(name, epi, kw, [kw["out"]])
    for M in (4128, 2064):
        (qa, sa), (qw, sw) = _lib.mx_quantize(rnd(g, M, 1024, scale=2.0)), _lib.mx_quantize(rnd(g, 1024, 1024, scale=1 / 32))
        kw = dict(a=qa, w=qw, bias=rnd(g, 1024), a_scale=sa, w_scale=sw, out=torch.empty(M, 1024, device="cuda", dtype=BF))
        _lib.gemm_ex(_lib.EPI_BF16, **kw)
        report(f"fp8 {M}x1024x1024", _lib.EPI_BF16, kw, [kw["out"]])
    pair = []
    for M in (4133, 4200):
        pair.append(dict(a=rnd(g, M, 512).to(BF), w=rnd(g, 512, 512, scale=512 ** -0.5).to(BF), bias=rnd(g, 512),
                         out=torch.empty(M, 512, device="cuda", dtype=BF), res_in=rnd(g, M, 512).to(BF), accumulate=True,
                         stats_out=torch.empty(M, 2, 2, device="cuda")))
    _lib.gemm_pair(_lib.EPI_RES, *pair)
    report("pair 4133+4200 x512x512", _lib.EPI_RES, pair[0], [p[k] for p in pair for k in ("out", "stats_out")],
           second=pair[1])
    # ---- block Linears: (config, D, rows of one bench lane, MXFP8)
    for cfg, D, rows, fp8 in (("cifar10_S", 512, 2 * 257, False), ("t2i_S x", 512, 32 * 334, False),
                              ("t2i_S m", 512, 32 * 590, False), ("t2i_S_512 x", 512, 10 * 1102, False),
                              ("t2i_S_512 m", 512, 10 * 2126, False), ("L/2", 1024, 50 * 258, False),
                              ("H/2", 1152, 50 * 258, False), ("H/4 fp8", 1152, 50 * 258, True)):
        for kind, N, K in (("qkv", 3 * D, D), ("proj", D, D), ("fc1", 4 * D, D), ("fc2", D, 4 * D), ("skip", D, 2 * D)):
            linear(f"{cfg} {kind} {rows}x{N}x{K}", rows, N, K, kind, g, fp8 and kind != "skip")
    # ---- the decoder's conv3x3 shapes at latent 32 (ch 128, ch_mult 1 2 4 4), 2 images: (H, Cin, N, up)
    for H, Cin, N, up in ((32, 512, 512, 0), (64, 512, 512, 1), (64, 512, 512, 0), (128, 512, 512, 1), (128, 512, 256, 0),
                          (128, 256, 256, 0), (256, 256, 256, 1), (256, 256, 128, 0), (256, 128, 128, 0)):
        x = rnd(g, 2, H >> up, H >> up, Cin).to(BF)
        w = rnd(g, N, Cin, 3, 3, scale=(9 * Cin) ** -0.5).to(BF)
        bias = rnd(g, N)
        for epi in (_lib.EPI_BF16, _lib.EPI_F32):
            out = _lib.gemm_conv3x3(x, w, bias, epi, up=up)
            ga = _lib.gemm_shape_args(2 * H * H, N, 9 * Cin, epi, conv_C=Cin) if HAS_PLAN else None
            report(f"conv {H}^2 {Cin}->{N} up {up} epi {epi}", epi, ga, [out], conv=(H, H, Cin, up))


if __name__ == "__main__":
    main()
