"""pdm_gemm_plan (every decision of the GEMM launcher as a pure host function) without a GPU.

Two independent statements of what the dispatcher did BEFORE the plan existed (csrc/gemm.hip at the parent commit:
gemm_launch, launch8s' stream-K / DUAL / MXO / grouped choices, fits_8s, fits_8s_mx, fits_rsrc, gemm_gn_fusable,
gemm_pair_groups), neither generated from the new function:

  (a) TABLE: hand-written rows -- every kernel family, the reachable error path, both post-passes, both split forms,
      the block Linears of every shipped config at the bench's row counts, and the corners nobody had written down;
  (b) ref_launch & co.: a statement-by-statement Python transcription of that host code, compared with the plan over
      a grid of shapes x epilogues x algos x operand options x policies.

Error paths: behind gemm_check (which pdm_gemm_plan runs, as every caller of gemm_launch does) only the no-store
timing mode's refusal is reachable; the MXFP8 >= 2 GiB refusal is gemm_check's own (asserted as PDM_ERR_ARG below), and
the half-N / tall guards and the missing-instantiation error stay behind rules that route those launches elsewhere.

One known, deliberate difference from the parent's gemm_gn_fusable: a conv wider than 512 pixels never fits the
descriptor kernels, is halved down to single images and ends on the 128 tile, which writes no GroupNorm partials; the
parent's hand mirror said "fusable" there (stale partials), the plan says no.  ref_gn_fusable carries that correction.
"""
import ctypes
import itertools
import os
import random
import re
from types import SimpleNamespace as NS

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16, GELU, F32, RES = 0, 1, 2, 3
LIM = 0x7fffffff
LDS = {"128": 65536, "ring32": 133120, "ring64": 133120, "8p": 133120, "8d": 135168, "8d_hn": 135168, "8t": 163840,
       "8s": 159760, "8g": 159760, "8s_mx": 163840, "mx": 155648}
M_2GIB = 4097 * 256   # bf16 rows of K = 1024 elements: 2 GiB + 512 KiB


@pytest.fixture(scope="module")
def lib():
    from panopticdiffusionmodels_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libpdm.so not built")
    L = _lib.load()
    L.pdm_set_gemm_tuning(0, 2)   # host state only: lets gemm_check pass a bf16 GEMM with no output (no-store mode)
    yield _lib
    L.pdm_set_gemm_tuning(0, 0)


# ---- cases: GemmArgs as capi.hip's to_gemm_args / to_plan_args builds them, on made-up addresses --------------------
def case(M, N, K, epi, conv=None, batch=0, a2=None, gather=False, fp8=False, out_fp8=False, ln=False, stats=False,
         out2=False, gn_P=0, mis=None, no_out=False, act=0, skf=False, acc=False, copy=False, keep_bf16=False):
    p = NS(A1=0x100000, lda1=K, A2=0, lda2=0, K1=K, W=0x200000, ldw=0, M=M, N=N, K=K, out_bf16=0, ldo=0, out_f32=0,
           ldr=0, accumulate=int(acc), a_rows_per_group=0, a_group_stride=0, batch=batch, conv=0, convH=0, convW=0,
           convC=0, conv_up=0, stats_out=0, stats_ld=(N + 255) // 256, ln_stats=0, ln_ld=(K + 255) // 256, ln_D=K,
           ln_colsum=0, fp8=int(fp8), a_scale=0, a_scale_ld=0, w_scale=0, w_scale_ld=0, out_fp8=0, ldo8=0, out_scale=0,
           out_scale_ld=0, mx_center=0, ln_gcol=0, res_in=0, ldri=0, out2=0, out2_rpg=0, out2_gs=0, stats_out2=0,
           res_f32=0, ldrf=0, act=act, sk_flags=int(skf), gn_P=gn_P, gn_cpg=N // 32 if gn_P else 0, dbg_tile0=0)
    if conv:
        H, W, C, up = conv
        p.conv, p.convH, p.convW, p.convC, p.conv_up = 1, H, W, C, up
        p.lda1, p.K, p.K1, p.ln_D, p.ln_ld = C, 9 * C, 9 * C, 9 * C, (9 * C + 255) // 256
    if a2:
        p.K1 = max(64, K // 128 * 64)
        p.A2 = 0x300000
        p.lda1, p.lda2 = (K, K) if a2 == "eq" else (p.K1, K - p.K1 + 8)
    if gather:
        p.a_rows_per_group, p.a_group_stride = 100, 120
    if fp8:
        p.a_scale, p.a_scale_ld, p.w_scale, p.w_scale_ld = 0x400000, M, 0x500000, N
    if out_fp8:
        p.out_fp8, p.ldo8, p.out_scale, p.out_scale_ld = 0x600000, N, 0x700000, M
    if ln:
        p.ln_stats, p.ln_colsum = 0x800000, 0x900000
        if fp8:
            p.ln_gcol = 0xa00000
    if stats:
        p.stats_out = 0xb00000
    if epi in (BF16, GELU, RES):
        if not (no_out or (out_fp8 and not keep_bf16)):
            p.out_bf16, p.ldo = 0xc00000, N
        if epi == RES and acc:
            p.res_in, p.ldri = 0xd00000, N
    else:
        p.out_f32, p.ldr = 0xe00000, N
        if copy:
            p.out_bf16, p.ldo = 0xc00000, N
    if out2:
        p.out2, p.out2_rpg, p.out2_gs = 0xf00000, 100, 120
        p.stats_out2 = 0xf80000 if stats else 0
    if mis == "bf16" and p.out_bf16:
        p.out_bf16 += 8
    if mis == "f32" and p.out_f32:
        p.out_f32 += 4
    if mis == "ldo" and p.out_bf16:
        p.ldo += 4
    return p


def to_c(_lib, p):
    g = _lib.PdmGemmArgs()
    for f in ("A1", "lda1", "A2", "lda2", "K1", "W", "ldw", "M", "N", "K", "out_bf16", "ldo", "out_f32", "ldr",
              "accumulate", "stats_out", "ln_stats", "ln_colsum", "fp8", "a_scale", "a_scale_ld", "w_scale",
              "w_scale_ld", "out_fp8", "ldo8", "out_scale", "out_scale_ld", "mx_center", "ln_gcol", "res_in", "ldri",
              "res_f32", "ldrf", "a_rows_per_group", "a_group_stride", "out2", "stats_out2"):
        v = getattr(p, f)
        setattr(g, f, (v or None) if dict(_lib.PdmGemmArgs._fields_)[f] is ctypes.c_void_p else v)
    g.out2_rows_per_group, g.out2_group_stride, g.ln_eps = p.out2_rpg, p.out2_gs, 1e-5
    return g


POLICY = dict(algo=0, sk=0, raster=0, dbg=0, mx_res_persist=1, ncu=256, persist_ok=1)


def query(_lib, p, epi, second=None, **pol):
    """The plan, or None where gemm_check rejects the arguments."""
    g = dict(POLICY, **pol)
    conv = (p.convH, p.convW, p.convC, p.conv_up) if p.conv else None
    try:
        return _lib.gemm_plan(to_c(_lib, p), epi, to_c(_lib, second) if second is not None else None, conv=conv,
                              batch=p.batch, act=p.act, gn_P=p.gn_P, sk_attached=bool(p.sk_flags), algo=g["algo"],
                              sk_mode=g["sk"], raster=g["raster"], dbg=g["dbg"], mx_res_persist=g["mx_res_persist"],
                              ncu=g["ncu"], persist_ok=g["persist_ok"])
    except ValueError:   # PDM_ERR_ARG
        return None


# ---- (b) the parent's host code, statement by statement --------------------------------------------------------------
def ref_fits_rsrc(p):
    es = 1 if p.fp8 else 2
    if p.conv:
        a1 = (p.M // (p.convH * p.convW)) * (p.convH >> p.conv_up) * (p.convW >> p.conv_up) * p.convC * 2
    elif p.a_rows_per_group > 0:
        a1 = ((p.M - 1) // p.a_rows_per_group * p.a_group_stride + p.a_rows_per_group) * p.lda1 * es
    else:
        a1 = p.M * p.lda1 * es
    a2 = p.M * p.lda2 * 2 if p.A2 else 0
    w = p.N * (p.ldw if p.ldw > 0 else p.K) * es
    return a1 < LIM and a2 < LIM and w < LIM and (
        not p.conv or (p.convW <= 512 and p.convH <= 512 and p.M // (p.convH * p.convW) < 8192))


def ref_fits_8s(p, epi, G):
    if not G["persist_ok"]:
        return False
    if epi not in (BF16, GELU, RES):
        return False
    if p.conv or p.batch > 1 or p.a_rows_per_group > 0 or p.fp8 or p.mx_center or p.out2:
        return False
    if p.out_fp8:
        if epi == RES or p.out_bf16 or not p.out_scale or p.N % 32 or p.ldo8 % 16 or p.out_scale_ld < p.M:
            return False
        if p.M * p.ldo8 >= LIM or ((p.N + 127) >> 7) * p.out_scale_ld * 4 >= LIM:
            return False
        if epi == GELU and p.act:
            return False
        if p.K < 256 or (p.A2 and p.K1 < p.K and p.lda2 != p.lda1) or (p.ln_stats and p.ln_ld > 8):
            return False
        if p.dbg_tile0 & 15:
            return False
        return ref_fits_rsrc(p)
    if not p.out_bf16:
        return False
    if epi == GELU and p.act:
        return False
    if (p.K < 256 or (p.A2 and p.K1 < p.K and p.lda2 != p.lda1) or p.N % 8 or p.ldo % 8 or (p.out_bf16 & 15) or
            (p.ln_stats and p.ln_ld > 8)):
        return False
    if p.M * p.ldo * 2 >= LIM:
        return False
    if epi == RES and p.accumulate and (p.ldri % 8 or (p.res_in & 15) or p.M * p.ldri * 2 >= LIM):
        return False
    if p.stats_out and p.M * p.stats_ld * 8 >= LIM:
        return False
    if p.dbg_tile0 & 15:
        return False
    return ref_fits_rsrc(p)


def ref_fits_8s_mx(p, epi, G):
    if not G["persist_ok"]:
        return False
    if (epi not in (BF16, RES) or not p.fp8 or p.out_fp8 or p.mx_center or p.A2 or p.K1 != p.K or p.conv or
            p.batch > 1 or p.a_rows_per_group > 0 or p.out2):
        return False
    if not p.out_bf16 or p.N % 8 or p.ldo % 8 or (p.out_bf16 & 15) or p.K % 128 or p.K < 512:
        return False
    if p.ln_stats and p.ln_ld > 8:
        return False
    if p.M * p.ldo * 2 >= LIM or (p.dbg_tile0 & 15):
        return False
    if epi == RES and p.accumulate and (p.ldri % 8 or (p.res_in & 15) or p.M * p.ldri * 2 >= LIM):
        return False
    if p.stats_out and p.M * p.stats_ld * 8 >= LIM:
        return False
    return ref_fits_rsrc(p)


def out(family, p, epi, bm, bn, block, conv=0, sched=0, mxo=0, sk=0, fp8=0, dual=0, batched=True):
    tn = (p.N + bn - 1) // bn
    nwg = (p.M + bm - 1) // bm * tn
    return NS(error=None, family=family, epi=epi, conv=conv, sched=sched, mxo=mxo, sk=sk, fp8=fp8, dual=dual,
              grid_x=nwg, grid_y=p.batch if batched and p.batch > 1 else 1, block=block, lds_bytes=LDS[family],
              tiles_n=tn, ntiles=nwg, nt0=nwg, raster=p.raster, split_m1=0, rowstats=False, out2_copy=False, parts=None)


ERR = NS(error="invalid", family=None, split_m1=0, parts=None)


def ref_launch8s(p, epi, G, p2=None):
    tn = (p.N + 255) // 256
    nt0 = (p.M + 255) // 256 * tn
    ntiles = nt0 + ((p2.M + 255) // 256 * tn if p2 else 0)
    grid = min(ntiles, G["ncu"])
    sk = False
    if (not p2 and p.sk_flags and G["sk"] and ntiles > grid and grid <= 256 and grid >= 8 and ntiles % grid):
        nk, gx, tmin = p.K // 64, (grid + 7) // 8, ntiles // 8
        waves = (ntiles + grid - 1) // grid
        fill = ntiles / (waves * grid)
        sk = tmin * nk >= gx * (nk + 4) and (G["sk"] == 2 or fill < 0.97)
    r = out("8s", p, epi, 256, 256, 512)
    r.grid_x, r.grid_y, r.ntiles, r.nt0 = grid, 1, ntiles, ntiles
    if sk:
        r.sk, r.dual = 1, 1
        if p.out_fp8:
            if epi not in (BF16, GELU):
                return ERR
            r.mxo = 1
            return r
        return r if epi in (BF16, GELU, RES) else ERR
    dual = int(bool(p.A2 and p.K1 < p.K))
    r.dual = dual
    if p.out_fp8:
        if epi not in (BF16, GELU):
            return ERR
        r.mxo = 1
        return r
    if p2:
        r.family, r.nt0 = "8g", nt0
    return r if epi in (BF16, GELU, RES) else ERR


def ref_launch(args, epi, G):
    """gemm_launch of the parent commit: what it launched, as the fields of a plan."""
    p = NS(**vars(args))
    p.raster = G["raster"] if G["raster"] else (8 if p.N >= 8 * 256 else 0)
    p.dbg_tile0 = G["dbg"]
    algo = G["algo"]
    rows_all = p.M * (p.batch if p.batch > 1 else 1)
    if algo == 0:
        algo = 7 if (rows_all >= 4096 and p.N >= 256) else (
            9 if (rows_all >= 65536 and p.N > 96 and p.N <= 128 and p.batch <= 1) else 1)
        if algo == 7 and ref_fits_8s(p, epi, G):
            algo = 11
    if algo == 11:
        if not p.fp8 and ref_fits_8s(p, epi, G):
            return ref_launch8s(p, epi, G)
        algo = 7
    if algo in (8, 9) and (p.N > 128 or epi not in (BF16, F32) or p.ln_stats or p.stats_out or p.out_fp8 or
                           p.a_rows_per_group > 0 or (algo == 9 and p.batch > 1)):
        algo = 1
    if epi in (BF16, GELU) and (p.N % 8 or p.ldo % 8 or (p.out_bf16 & 15)):
        algo = 1
    if epi == F32 and (p.N % 8 or p.ldr % 4 or (p.out_f32 & 15) or (p.out_bf16 and (p.ldo % 8 or (p.out_bf16 & 15)))):
        algo = 1
    if p.fp8:
        if not ref_fits_rsrc(p):
            return ERR
        if (G["algo"] == 11 or (G["algo"] == 0 and G["mx_res_persist"] and p.M >= 4096)) and ref_fits_8s_mx(p, epi, G):
            r = out("8s_mx", p, RES if epi == RES else BF16, 256, 256, 512, fp8=1)
            r.grid_x, r.grid_y = min(r.ntiles, G["ncu"]), 1
            return r
        return out("mx", p, epi, 256, 256, 512, fp8=1, batched=False)
    if p.out_fp8:
        algo = 7
    if epi in (BF16, GELU) and not p.out_bf16 and not p.out_fp8:
        if not ref_fits_rsrc(p) or p.conv or p.batch > 1:
            return NS(error="nostore", family=None, split_m1=0, parts=None)
        algo = 7
    if algo >= 5 and not ref_fits_rsrc(p) and p.batch <= 1 and p.a_rows_per_group == 0 and not p.out_fp8:
        hw = p.convH * p.convW if p.conv else 1
        m1 = (p.M // hw // 2) * hw if p.conv else ((p.M // 2 + 255) // 256) * 256
        if 0 < m1 < p.M:
            a, b = ref_parts(args, m1)
            ra, rb = ref_launch(a, epi, G), ref_launch(b, epi, G)
            return NS(error=ra.error or rb.error, split_m1=m1, parts=(ra, rb), out2_copy=bool(p.out2), rowstats=False,
                      family=ra.family)
    conv = 1 if p.conv else 0
    if algo == 8 and ref_fits_rsrc(p):
        if p.N > 128 or epi not in (BF16, F32):
            return ERR
        return out("8d_hn", p, epi, 256, 128, 512, conv=conv, sched=2)
    if algo == 9 and ref_fits_rsrc(p):
        if p.N > 128 or p.batch > 1 or epi not in (BF16, F32):
            return ERR
        return out("8t", p, epi, 512, 128, 512, conv=conv, batched=False)
    if algo in (8, 9):
        algo = 1
    if epi == RES:
        if algo != 1 and ref_fits_rsrc(p):
            return out("8d", p, RES, 256, 256, 512, conv=0, sched=2)
        algo = 1
    if algo >= 5 and ref_fits_rsrc(p):
        return out("8d", p, epi, 256, 256, 512, conv=conv, sched=0 if algo == 5 else 1 if algo == 6 else 2)
    if algo >= 5:
        algo = 3
    if algo == 2 and p.K % 32 == 0:
        return out("ring32", p, epi, 256, 256, 512)
    if algo == 4 and p.K % 128 == 0:
        return out("8p", p, epi, 256, 256, 512, conv=conv)
    if algo in (3, 4) and p.K % 64 == 0:
        return out("ring64", p, epi, 256, 256, 512)
    r = out("128", p, epi, 128, 128, 256)
    r.rowstats = bool(p.stats_out and p.batch <= 1)
    r.out2_copy = bool(epi == RES and p.out2)
    return r


def ref_parts(args, m1):
    """The two parts of the parent's row split.  Their operand pointers advance by whole 16-byte multiples (lda % 8,
    m1 a multiple of 256 rows or of whole images), so only M, the flags and the second output change."""
    a, b = NS(**vars(args)), NS(**vars(args))
    a.sk_flags = b.sk_flags = 0
    a.out2 = b.out2 = a.stats_out2 = b.stats_out2 = 0
    a.M, b.M = m1, args.M - m1
    return a, b


def ref_gn_fusable(p, epi, G):
    if G["algo"] != 0 or epi not in (F32, BF16) or not (p.conv or epi == F32):
        return False
    if p.fp8 or p.out_fp8 or p.batch > 1 or p.a_rows_per_group > 0 or p.ln_stats or p.stats_out or p.A2:
        return False
    if p.gn_P <= 0 or p.gn_P % 256 or p.M % p.gn_P or p.N % 32 or p.gn_cpg * 32 != p.N:
        return False
    if p.gn_cpg not in (4, 8, 16, 32):
        return False
    a7, a9 = p.M >= 4096 and p.N >= 256, p.M >= 65536 and p.N > 96 and p.N <= 128
    if not a7 and not a9:
        return False
    if epi == BF16 and (p.N % 8 or p.ldo % 8 or (p.out_bf16 & 15) or not p.out_bf16):
        return False
    if epi == F32 and (p.N % 8 or p.ldr % 4 or (p.out_f32 & 15) or (p.out_bf16 and (p.ldo % 8 or (p.out_bf16 & 15)))):
        return False
    if not (ref_fits_rsrc(p) or p.conv):
        return False
    return not (p.conv and (p.convW > 512 or p.convH > 512))   # the correction of the module docstring


def ref_pair_groups(p, q, epi, G):
    """gemm_pair_groups as gemm_launch_pair called it (raster and the dbg bits set on both problems)."""
    p, q = NS(**vars(p)), NS(**vars(q))
    p.dbg_tile0 = q.dbg_tile0 = G["dbg"]
    algo_ok = G["algo"] in (0, 11)
    same = (p.N == q.N and p.K == q.K and p.K1 == q.K1 and p.lda1 == q.lda1 and p.ldw == q.ldw and p.ldo == q.ldo and
            p.ldri == q.ldri and p.accumulate == q.accumulate and p.stats_ld == q.stats_ld and p.ln_ld == q.ln_ld and
            p.ln_D == q.ln_D and (not p.ln_stats) == (not q.ln_stats) and (not p.stats_out) == (not q.stats_out) and
            (not p.A2) == (not q.A2) and (not p.A2 or p.lda2 == q.lda2) and not p.out_fp8 and not q.out_fp8)
    return bool(algo_ok and same and p.M >= 4096 and q.M >= 4096 and p.N >= 256 and ref_fits_8s(p, epi, G) and
                ref_fits_8s(q, epi, G))


FIELDS = ("family", "epi", "conv", "sched", "mxo", "sk", "fp8", "dual", "grid_x", "grid_y", "block", "lds_bytes",
          "tiles_n", "ntiles", "nt0", "raster", "rowstats", "out2_copy")


def compare(_lib, p, epi, G, seen, depth=0):
    """Plan == transcription for one case (and, recursively, for the parts of a split); False if gemm_check rejects."""
    pl = query(_lib, p, epi, **G)
    if pl is None:
        return False
    ref = ref_launch(p, epi, G)
    ctx = (vars(p), epi, G, pl, ref)
    assert bool(pl.error) == bool(ref.error), ctx
    assert pl.gn_fusable == ref_gn_fusable(p, epi, G), ctx
    assert pl.writes_gn or not pl.gn_fusable, ctx
    if ref.error:
        assert ref.parts or ref.error == "invalid" or pl.error == ref.error, ctx
        seen.add(("error", pl.error))
        return True
    assert pl.split_m1 == ref.split_m1 and pl.family == ref.family, ctx
    if ref.parts:
        assert pl.out2_copy == ref.out2_copy and not pl.rowstats and depth < 12, ctx
        seen.add(("split", "conv" if p.conv else "rows"))
        for part in ref_parts(p, ref.split_m1):
            assert compare(_lib, part, epi, G, seen, depth + 1), ctx
        return True
    for f in FIELDS:
        assert getattr(pl, f) == getattr(ref, f), (f, ctx)
    seen.update({("family", pl.family), ("rowstats", pl.rowstats), ("out2_copy", pl.out2_copy),
                 ("writes_gn", pl.writes_gn), ("sk", pl.sk), ("dual", pl.dual), ("mxo", pl.mxo)})
    return True


MS = (1, 255, 256, 4095, 4096, 4133, 65535, 65536, 1100000, M_2GIB)
NS_ = (4, 96, 100, 120, 128, 132, 256, 264, 1000, 2048, 2056)
KS = (64, 128, 192, 256, 512, 1024, 1152)
ALGOS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11)
OPTIONS = (
    {}, dict(batch=4), dict(batch=70), dict(a2="eq"), dict(a2="ne"), dict(gather=True), dict(fp8=True),
    dict(fp8=True, ln=True), dict(fp8=True, out_fp8=True, keep_bf16=True), dict(out_fp8=True),
    dict(out_fp8=True, keep_bf16=True), dict(ln=True), dict(stats=True), dict(stats=True, acc=True), dict(out2=True),
    dict(out2=True, stats=True), dict(gn_P=256), dict(gn_P=256, copy=True), dict(mis="bf16"), dict(mis="f32"),
    dict(mis="ldo"), dict(mis="bf16", copy=True), dict(no_out=True), dict(act=1), dict(skf=True), dict(skf=True, a2="eq"),
    dict(skf=True, out_fp8=True), dict(conv=(16, 16, 64, 0), gn_P=256), dict(conv=(32, 32, 128, 1), gn_P=1024),
    dict(conv=(16, 16, 64, 0), no_out=True), dict(conv=(16, 1024, 64, 0), gn_P=16384), dict(conv=(16, 16, 64, 0)),
)
POLICIES = (
    {}, dict(sk=1), dict(sk=2), dict(sk=2, ncu=8), dict(sk=1, ncu=64), dict(dbg=1), dict(dbg=2), dict(dbg=16), dict(dbg=128),
    dict(ncu=24), dict(persist_ok=0), dict(mx_res_persist=0), dict(raster=4),
)


def conv_rows(o, M):
    """A conv case's row count: whole images, about M rows."""
    H, W = o["conv"][:2]
    return max(1, M // (H * W)) * H * W


def test_transcription_equals_plan_over_the_grid(lib):
    seen, n = set(), 0
    # every shape x epilogue x algo on plain operands, then a seeded sample of the full product with the options
    plain = [(M, N, K, epi, algo, {}, {}) for M, N, K, epi, algo in itertools.product(MS, NS_, KS, range(4), ALGOS)]
    rng = random.Random(20240607)
    full = [(rng.choice(MS), rng.choice(NS_), rng.choice(KS), rng.randrange(4), rng.choice(ALGOS), rng.choice(OPTIONS),
             rng.choice(POLICIES)) for _ in range(25000)]
    # the corners a sample may miss: every option x every policy on the persistent shapes, both split forms
    corners = [(M, N, K, epi, algo, o, g) for o in OPTIONS for g in POLICIES for epi in range(4) for algo in (0, 9, 11)
               for M, N, K in ((4133, 1000, 1024), (65536, 128, 64), (M_2GIB, 256, 1024), (8192 * 256, 256, 64),
                               (70000, 2048, 512))]
    for M, N, K, epi, algo, o, g in plain + full + corners:
        if "conv" in o:
            M = conv_rows(o, M)
        p = case(M, N, K, epi, **o)
        n += compare(lib, p, epi, dict(POLICY, algo=algo, **g), seen)
    assert n > 30000, n
    # the grid cannot go hollow unnoticed
    fams = {v for k, v in seen if k == "family"}
    assert fams == set(lib.GEMM_FAMILIES) - {"8g"}, fams          # 8g: the pair test below
    assert ("error", "nostore") in seen
    assert {("split", "conv"), ("split", "rows")} <= seen
    for flag in ("rowstats", "out2_copy", "writes_gn", "sk", "dual", "mxo"):
        assert {v for k, v in seen if k == flag} == {0, 1} or {v for k, v in seen if k == flag} == {False, True}, flag


def test_pairing_equals_transcription(lib):
    grouped = set()
    for (Mp, Mq), N, K, epi, algo, g, o, oq in itertools.product(
            ((4133, 4200), (4096, 4095), (258, 4200), (70000, 4133)), (96, 256, 1000, 2056), (128, 256, 1024),
            (BF16, GELU, RES, F32), (0, 1, 7, 11), ({}, dict(dbg=1), dict(persist_ok=0), dict(sk=2)),
            ({}, dict(a2="eq"), dict(a2="ne"), dict(ln=True), dict(stats=True, acc=True), dict(out_fp8=True),
             dict(skf=True), dict(mis="ldo")),
            (None, {}, dict(ln=True))):
        p, q = case(Mp, N, K, epi, **o), case(Mq, N, K, epi, **(o if oq is None else oq))
        G = dict(POLICY, algo=algo, **g)
        pl = query(lib, p, epi, second=q, **G)
        if pl is None:
            continue
        want = ref_pair_groups(p, q, epi, G)
        assert pl.grouped == want, (vars(p), vars(q), epi, G, pl)
        grouped.add(want)
        if want:
            ref = ref_launch8s(NS(**vars(p), raster=0), epi, G, q)
            assert (pl.family, pl.dual, pl.grid_x, pl.ntiles, pl.nt0, pl.lds_bytes, pl.sk) == \
                ("8g", ref.dual, ref.grid_x, ref.ntiles, ref.nt0, LDS["8g"], 0), (pl, ref)
        else:   # two launches: the first problem's own plan, without the pair's stream-K state
            one = NS(**vars(p))
            one.sk_flags = 0
            ref = ref_launch(one, epi, G)
            assert pl.family == ref.family and bool(pl.error) == bool(ref.error)
    assert grouped == {True, False}


# ---- (a) the hand-written table ---------------------------------------------------------------------------------------
def lin(M, N, K, epi, **o):
    return case(M, N, K, epi, **o)


# bench rows: imagenet256 L / H (50-row lanes of 258 tokens), imagenet512 H fp8 (the same token count at patch 4),
# cifar10 S (lanes of 2 x 257 tokens x ...), mscoco t2i S (334 image-stream and 590 mask-stream tokens per row)
R = 50 * 258
# (name, case, epi, policy, expected fields)
TABLE = [
    # ---- one row per family
    ("128: small M", lin(515, 768, 2048, BF16), BF16, {}, dict(family="128", block=256, grid_x=5 * 6, lds_bytes=65536)),
    ("ring32: algo 2", lin(4096, 256, 256, BF16), BF16, dict(algo=2), dict(family="ring32", grid_x=16)),
    ("ring64: algo 3", lin(4096, 256, 256, F32), F32, dict(algo=3), dict(family="ring64", epi=F32)),
    ("8p: algo 4, K % 128 == 0", lin(4096, 256, 256, GELU), GELU, dict(algo=4), dict(family="8p", epi=GELU)),
    ("8p needs K % 128: ring64", lin(4096, 256, 192, GELU), GELU, dict(algo=4), dict(family="ring64")),
    ("8d: fp32 epilogue, automatic", lin(4133, 1024, 1024, F32), F32, {}, dict(family="8d", sched=2, grid_x=17 * 4)),
    ("8d sched 0: algo 5", lin(4096, 256, 256, BF16), BF16, dict(algo=5), dict(family="8d", sched=0)),
    ("8d sched 1: algo 6", lin(4096, 256, 256, BF16), BF16, dict(algo=6), dict(family="8d", sched=1)),
    ("8d conv", case(4096, 256, 576, F32, conv=(32, 32, 64, 0)), F32, {}, dict(family="8d", conv=1, sched=2, grid_x=16)),
    ("8d_hn: algo 8", lin(4096, 128, 256, BF16), BF16, dict(algo=8), dict(family="8d_hn", sched=2, tiles_n=1, grid_x=16)),
    ("8t: tall, automatic", lin(65536, 128, 64, BF16), BF16, {}, dict(family="8t", grid_x=128, grid_y=1, lds_bytes=163840)),
    ("8s: GELU, automatic", lin(4133, 1000, 1024, GELU), GELU, {}, dict(family="8s", epi=GELU, dual=0, grid_x=68, ntiles=68)),
    ("8s: one workgroup per tile below the CU count", lin(R, 1024, 1024, BF16), BF16, {}, dict(family="8s", grid_x=204, ntiles=51 * 4)),
    ("8s: grid capped at the CUs", lin(70000, 1024, 1024, BF16), BF16, {}, dict(family="8s", grid_x=256, ntiles=274 * 4)),
    ("8s_mx: fp8 bf16 epilogue", lin(4128, 1024, 1024, BF16, fp8=True), BF16, {}, dict(family="8s_mx", fp8=1, grid_x=68)),
    ("mx: fp8 below 4096 rows", lin(2064, 1024, 1024, BF16, fp8=True), BF16, {}, dict(family="mx", fp8=1, grid_x=36)),
    # ---- the corners
    ("algo 11 + fp32 epilogue: 8d sched 2", lin(4133, 1024, 1024, F32), F32, dict(algo=11), dict(family="8d", sched=2)),
    ("algo 8 with N > 128: the 128 tile", lin(4096, 256, 256, BF16), BF16, dict(algo=8), dict(family="128")),
    ("algo 9 with N > 128: the 128 tile", lin(65536, 132, 256, F32), F32, dict(algo=9), dict(family="128")),
    ("EPI_RES under algo 5: 8d<0, 2>", lin(4096, 256, 256, RES), RES, dict(algo=5), dict(family="8d", epi=RES, sched=2, conv=0)),
    ("EPI_RES under algo 6: 8d<0, 2>", lin(4096, 256, 256, RES), RES, dict(algo=6), dict(family="8d", epi=RES, sched=2)),
    ("EPI_RES under algo 3: 8d<0, 2> too", lin(4096, 256, 256, RES), RES, dict(algo=3), dict(family="8d", epi=RES, sched=2)),
    ("EPI_RES under algo 1: the 128 tile", lin(4096, 256, 256, RES), RES, dict(algo=1), dict(family="128", epi=RES)),
    ("misaligned out_bf16: the 128 tile", lin(4133, 1024, 1024, BF16, mis="bf16"), BF16, {}, dict(family="128")),
    ("ldo % 8: the 128 tile", lin(4133, 1024, 1024, GELU, mis="ldo"), GELU, dict(algo=7), dict(family="128")),
    ("out_fp8 forces the 256-tile epilogue", lin(256, 128, 128, BF16, out_fp8=True), BF16, {}, dict(family="8d", sched=2)),
    ("out_fp8 beside out_bf16: not persistent", lin(4133, 1024, 1024, BF16, out_fp8=True, keep_bf16=True), BF16, {},
     dict(family="8d")),
    ("out_fp8 alone: persistent MXO", lin(4133, 1024, 1024, GELU, out_fp8=True), GELU, {}, dict(family="8s", mxo=1)),
    ("fp8 under algo 11 below 4096 rows: 8s_mx", lin(2064, 1024, 1024, BF16, fp8=True), BF16, dict(algo=11), dict(family="8s_mx")),
    ("fp8 GELU: no persistent form", lin(4128, 1024, 1024, GELU, fp8=True), GELU, {}, dict(family="mx", epi=GELU)),
    ("fp8 K < 512: mx", lin(4128, 1024, 256, BF16, fp8=True), BF16, {}, dict(family="mx")),
    ("fp8 with mx_res_persist off: mx", lin(4128, 1024, 1024, RES, fp8=True), RES, dict(mx_res_persist=0), dict(family="mx")),
    ("K < 256: not persistent", lin(4133, 1024, 192, BF16), BF16, {}, dict(family="8d")),
    ("quick GELU: not persistent", lin(4133, 1024, 1024, GELU, act=1), GELU, {}, dict(family="8d", epi=GELU)),
    ("row gather: not persistent", lin(4100, 1024, 1024, BF16, gather=True), BF16, {}, dict(family="8d")),
    ("a spilling build: algo 7", lin(4133, 1024, 1024, BF16), BF16, dict(persist_ok=0), dict(family="8d", sched=2)),
    ("split-K, equal lda: DUAL", lin(4133, 1024, 2048, RES, a2="eq"), RES, {}, dict(family="8s", dual=1)),
    ("split-K, unequal lda: 8d", lin(4133, 1024, 2048, RES, a2="ne"), RES, {}, dict(family="8d", epi=RES)),
    ("batched counts all rows", lin(1024, 1024, 64, F32, batch=4), F32, {}, dict(family="8d", grid_x=16, grid_y=4)),
    ("batched, tall shape: no 8t", lin(65536, 128, 64, F32, batch=2), F32, {}, dict(family="128", grid_y=2)),
    ("raster 8 from 8 column tiles", lin(4133, 2048, 1024, BF16), BF16, {}, dict(family="8s", raster=8)),
    ("raster override", lin(4133, 1024, 1024, BF16), BF16, dict(raster=4), dict(family="8s", raster=4)),
    # ---- stream-K: only with flags attached, ntiles % grid != 0, grid >= 8 and the share rule
    ("sk: taken", lin(70000, 1024, 1024, BF16, skf=True), BF16, dict(sk=2), dict(family="8s", sk=1, dual=1, ntiles=1096)),
    ("sk: no flags", lin(70000, 1024, 1024, BF16), BF16, dict(sk=2), dict(family="8s", sk=0)),
    ("sk: policy off", lin(70000, 1024, 1024, BF16, skf=True), BF16, dict(sk=0), dict(family="8s", sk=0)),
    ("sk: whole waves (1024 tiles)", lin(65536, 1024, 1024, BF16, skf=True), BF16, dict(sk=2), dict(sk=0, ntiles=1024)),
    ("sk: one wave", lin(4133, 1024, 1024, BF16, skf=True), BF16, dict(sk=2), dict(sk=0, grid_x=68)),
    ("sk: grid < 8", lin(4133, 1024, 1024, BF16, skf=True), BF16, dict(sk=2, ncu=7), dict(sk=0, grid_x=7)),
    ("sk: share rule (tmin nk < gx (nk + 4))", lin(4133, 1024, 256, BF16, skf=True), BF16, dict(sk=2, ncu=64),
     dict(sk=0, grid_x=64, ntiles=68)),   # 8 * 4 < 8 * 8
    ("sk auto: last wave >= 97 % full", lin(130000, 1024, 1024, BF16, skf=True), BF16, dict(sk=1), dict(sk=0, ntiles=2032)),
    ("sk auto: taken below", lin(70000, 1024, 1024, BF16, skf=True), BF16, dict(sk=1), dict(sk=1)),
    ("sk with the MXFP8 copy", lin(70000, 1024, 1024, GELU, skf=True, out_fp8=True), GELU, dict(sk=2), dict(sk=1, mxo=1, dual=1)),
    # ---- post-passes
    ("row stats behind the 128 tile", lin(515, 768, 2048, F32, stats=True), F32, {}, dict(family="128", rowstats=True)),
    ("no row stats on the 256 tile", lin(4133, 768, 2048, F32, stats=True), F32, {}, dict(family="8d", rowstats=False)),
    ("out2 copied behind the 128 tile", lin(515, 768, 2048, RES, out2=True), RES, {}, dict(family="128", out2_copy=True)),
    ("out2 stored by the 256-tile epilogue", lin(4133, 768, 2048, RES, out2=True), RES, {}, dict(family="8d", out2_copy=False)),
    # ---- GroupNorm partials
    ("gn: fp32 Linear on 8d", lin(4096, 512, 512, F32, gn_P=1024), F32, {}, dict(family="8d", writes_gn=True, gn_fusable=True)),
    ("gn: conv bf16 on 8d", case(4096, 256, 576, BF16, conv=(32, 32, 64, 0), gn_P=1024), BF16, {},
     dict(family="8d", writes_gn=True, gn_fusable=True)),
    ("gn: tall tile", lin(65536, 128, 64, F32, gn_P=4096), F32, {}, dict(family="8t", writes_gn=True, gn_fusable=True)),
    ("gn: bf16 Linear is persistent", lin(4096, 512, 512, BF16, gn_P=1024), BF16, {}, dict(family="8s", writes_gn=False)),
    ("gn: the 128 tile", lin(2048, 512, 512, F32, gn_P=1024), F32, {}, dict(family="128", writes_gn=False, gn_fusable=False)),
    ("gn: a forced algo", lin(4096, 512, 512, F32, gn_P=1024), F32, dict(algo=7), dict(family="8d", writes_gn=False)),
    ("gn: images of partial tiles", lin(4096 + 512, 512, 512, F32, gn_P=512 + 64), F32, {},
     dict(family="8d", writes_gn=True, gn_fusable=False)),
    # ---- splits past 2 GiB
    ("split: Linear rows", lin(M_2GIB, 256, 1024, BF16), BF16, dict(algo=7), dict(family="8d", split_m1=2049 * 256)),
    ("split: automatic, the parts are persistent again", lin(M_2GIB, 256, 1024, BF16), BF16, {}, dict(family="8s", split_m1=2049 * 256)),
    ("split: out2 copied once", lin(M_2GIB, 256, 1024, RES, out2=True), RES, {}, dict(split_m1=2049 * 256, out2_copy=True)),
    ("split: a Linear's parts are not whole images", lin(M_2GIB, 256, 1024, F32, gn_P=256), F32, {},
     dict(split_m1=2049 * 256, writes_gn=False, gn_fusable=False)),
    ("split: conv by whole images", case(8192 * 256, 256, 576, F32, conv=(16, 16, 64, 0), gn_P=256), F32, {},
     dict(family="8d", conv=1, split_m1=4096 * 256, writes_gn=True, gn_fusable=True)),
    ("no split under the 128 tile", lin(M_2GIB, 256, 1024, BF16), BF16, dict(algo=1), dict(family="128", split_m1=0)),
    ("no split of a gather: ring64", lin(M_2GIB, 256, 1024, BF16, gather=True), BF16, dict(algo=7), dict(family="ring64")),
    # ---- the reachable error path
    ("no-store mode on a conv", case(4096, 256, 576, BF16, conv=(32, 32, 64, 0), no_out=True), BF16, dict(dbg=2),
     dict(error="nostore", family=None)),
    ("no-store mode: 8d", lin(512, 256, 256, BF16, no_out=True), BF16, dict(dbg=2), dict(error=None, family="8d", sched=2)),
]
# ---- the block Linears of every shipped config at the bench's row counts (the persistent kernel on
# every bf16 block Linear from 4096 rows; the MXFP8 Linears of U-ViT-H on its MXFP8-operand form)
# rows of one of the bench's two lanes: half the config's mini_batch_size, doubled where cfg_scale > 0, times the tokens
for name, D, rows, fp8 in (("cifar10_uvit_small", 512, 2 * 257, False), ("imagenet256_uvit_large", 1024, R, False),
                           ("imagenet256_uvit_huge", 1152, R, False), ("imagenet512_uvit_huge", 1152, R, True),
                           ("mscoco_uvit_small x", 512, 32 * 334, False), ("mscoco_uvit_small m", 512, 32 * 590, False),
                           ("mscoco_uvit_small_512 x", 512, 10 * 1102, False),
                           ("mscoco_uvit_small_512 m", 512, 10 * 2126, False)):
    small = rows < 4096
    fam = "128" if small else "8s"
    famr = "128" if small else "8s"
    if not fp8:
        TABLE += [
            (f"{name} qkv", lin(rows, 3 * D, D, BF16, ln=True), BF16, {}, dict(family=fam, dual=0)),
            (f"{name} proj", lin(rows, D, D, RES, acc=True, stats=True), RES, {}, dict(family=famr, rowstats=small)),
            (f"{name} fc1", lin(rows, 4 * D, D, GELU, ln=True), GELU, {}, dict(family=fam, epi=GELU)),
            (f"{name} fc2", lin(rows, D, 4 * D, RES, acc=True, stats=True), RES, {}, dict(family=famr)),
            (f"{name} skip_linear", lin(rows, D, 2 * D, RES, a2="eq", stats=True), RES, {},
             dict(family=famr, dual=0 if small else 1)),
        ]
    else:
        TABLE += [
            (f"{name} qkv fp8", lin(rows, 3 * D, D, BF16, fp8=True, ln=True), BF16, {}, dict(family="8s_mx", epi=BF16)),
            (f"{name} proj fp8", lin(rows, D, D, RES, fp8=True, acc=True, stats=True), RES, {}, dict(family="8s_mx", epi=RES)),
            (f"{name} fc1 -> MXFP8", lin(rows, 4 * D, D, GELU, ln=True, out_fp8=True), GELU, {}, dict(family="8s", mxo=1)),
            (f"{name} fc2 fp8", lin(rows, D, 4 * D, RES, fp8=True, acc=True, stats=True), RES, {}, dict(family="8s_mx")),
            (f"{name} skip_linear", lin(rows, D, 2 * D, RES, a2="eq", stats=True), RES, {}, dict(family="8s", dual=1)),
        ]


@pytest.mark.parametrize("row", TABLE, ids=[r[0] for r in TABLE])
def test_hand_written_table(lib, row):
    name, p, epi, pol, want = row
    pl = query(lib, p, epi, **pol)
    assert pl is not None, "gemm_check rejected the case"
    want = dict({"error": None} if "error" not in want else {}, **want)
    got = {k: getattr(pl, k) for k in want}
    assert got == want, pl


def test_table_covers_every_family_error_and_pass():
    fams = {r[4].get("family") for r in TABLE}
    from panopticdiffusionmodels_amd import _lib
    assert fams >= set(_lib.GEMM_FAMILIES) - {"8g"}
    assert any(r[4].get("error") for r in TABLE) and any(r[4].get("rowstats") for r in TABLE)
    assert any(r[4].get("out2_copy") for r in TABLE) and any(r[4].get("split_m1") for r in TABLE)


def test_grouped_pair_is_8g(lib):
    p = lin(4133, 1024, 1024, RES, acc=True, stats=True)
    q = lin(4200, 1024, 1024, RES, acc=True, stats=True)
    pl = query(lib, p, RES, second=q)
    assert pl.grouped and pl.family == "8g" and pl.dual == 0 and pl.error is None
    assert (pl.nt0, pl.ntiles, pl.grid_x, pl.lds_bytes) == (17 * 4, 17 * 4 + 17 * 4, 136, 159760)
    small = lin(2000, 1024, 1024, RES, acc=True, stats=True)
    pl = query(lib, p, RES, second=small)
    assert not pl.grouped and pl.family == "8s" and pl.ntiles == 68      # each alone: the second is not persistent
    pl = query(lib, lin(4133, 1024, 2048, RES, a2="eq"), RES, second=lin(4200, 1024, 2048, RES, a2="eq"))
    assert pl.grouped and pl.family == "8g" and pl.dual == 1


def test_symbols_and_errors(lib):
    with open(os.path.join(REPO, "include", "pdm.h")) as f:
        header = f.read()
    assert re.search(r"\bint\s+pdm_gemm_plan\s*\(", header)
    names = re.findall(r"#define\s+PDM_GEMM_(?!ERR_|FAMILIES)(\w+)\s+(\d+)", header)
    assert [n.lower() for n, _ in names] == list(lib.GEMM_FAMILIES)
    assert [int(v) for _, v in names] == list(range(len(names)))
    assert int(re.search(r"#define\s+PDM_GEMM_FAMILIES\s+(\d+)", header).group(1)) == len(names)
    errs = re.findall(r"#define\s+PDM_GEMM_ERR_(\w+)\s+(\d+)", header)
    assert [n.lower() for n, _ in errs] == list(lib.GEMM_PLAN_ERRORS[1:])
    L = lib.load()
    out = (ctypes.c_int * 24)()
    o = lib.PdmGemmPlanOpts(ncu=256, persist_ok=1)
    g = to_c(lib, lin(256, 256, 256, BF16))
    assert L.pdm_gemm_plan(None, None, 0, ctypes.byref(o), out) == 1
    assert L.pdm_gemm_plan(ctypes.byref(g), None, 0, None, out) == 1
    assert L.pdm_gemm_plan(ctypes.byref(g), None, 0, ctypes.byref(o), None) == 1
    assert L.pdm_gemm_plan(ctypes.byref(g), None, 0, ctypes.byref(o), out) == 0 and out[1] == 0
    for bad in (dict(algo=10), dict(algo=12), dict(sk_mode=3), dict(raster=65)):
        assert L.pdm_gemm_plan(ctypes.byref(g), None, 0, ctypes.byref(lib.PdmGemmPlanOpts(ncu=256, persist_ok=1, **bad)),
                               out) == 1
    # gemm_check's refusals come back as PDM_ERR_ARG: an MXFP8 operand past 2 GiB, K % 64, a missing output
    big = to_c(lib, lin(M_2GIB * 2, 256, 1024, BF16, fp8=True))
    assert L.pdm_gemm_plan(ctypes.byref(big), None, 0, ctypes.byref(o), out) == 1 and b"2 GiB" in L.pdm_last_error()
    assert query(lib, lin(256, 256, 100, BF16), BF16) is None
    assert query(lib, lin(256, 256, 256, F32, no_out=True), RES) is None


def test_plan_is_pure(lib):
    """The same arguments and policy give the same plan whatever the process's knobs say, and asking changes none."""
    L = lib.load()
    p = lin(70000, 1024, 1024, BF16, skf=True)
    before = query(lib, p, BF16, sk=2)
    assert L.pdm_set_gemm_algo(1) == 0 and L.pdm_set_gemm_sk(1) == 0
    try:
        assert query(lib, p, BF16, sk=2) == before
        n0 = L.pdm_gemm_sk_launches()
        assert lib.gemm_plan(to_c(lib, p), BF16, dbg=0, ncu=256, persist_ok=1).family == "128"    # current: algo 1
        assert L.pdm_gemm_sk_launches() == n0
    finally:
        L.pdm_set_gemm_algo(0)
        L.pdm_set_gemm_sk(0)
    assert lib.gemm_plan(to_c(lib, p), BF16, dbg=0, ncu=256, persist_ok=1).family == "8s"
