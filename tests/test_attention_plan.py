"""pdm_attention_plan (the attention launcher's decisions as a pure host function) without a GPU.

The expected plans below are written by hand from the dispatcher as it stood before the plan query existed
(csrc/attention.hip, attention_launch), not generated from the new function:

  Dh 72: head-resident (h72) when (round8(L) + round16(L)) * 144 <= 80 KiB and round32(L) <= 2 * round8(L), i.e.
         L = 9 .. 280; the persistent h72p only under algos 14-16 and with >= 4 query tiles (L >= 49);
  Dh 64: head-resident while round32(L) * 256 <= 160 KiB (L <= 640), 4 waves while that is <= 80 KiB (L <= 320), else 8;
         the persistent v3 (automatic, algo 11) needs a query tile per wave (ceil(L / 16) >= waves), else v2;
         algo 10 = v2 with VALU row sums; algos 2 / 3 = kv kernels while ceil(ceil(L / 16) / T) <= 12 / 8 waves;
  tail1: L > 64 and L % 64 in 1 .. 16, on v3 and h72 only (their TK = 1 instantiations), never on a timing variant;
  everything else: the streamed kernel, 4 waves, no dynamic LDS, ceil(B H / 8) * 8 * ceil(ceil(L / 16) / 4) blocks.
"""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ARG = 0, 1
B, H = 2, 3


@pytest.fixture(scope="module")
def lib():
    from panopticdiffusionmodels_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libpdm.so not built")
    return _lib.load()


def plan(lib, L, Dh, algo=0, B=B, H=H, ncu=256):
    from panopticdiffusionmodels_amd import _lib
    assert lib is _lib.load()
    return _lib.attention_plan(B, L, H, Dh, algo, ncu)


def r(x, m):
    return (x + m - 1) // m * m


# (Dh, algo, L, family, waves or None, tail1)
TABLE = []
for L in (1, 16, 48):
    TABLE.append((64, 0, L, "v2", 4, False))
for L in (49, 64):
    TABLE.append((64, 0, L, "v3", 4, False))
for L in (65, 80, 258):
    TABLE.append((64, 0, L, "v3", 4, True))
for L in (81, 320):
    TABLE.append((64, 0, L, "v3", 4, False))
TABLE += [
    (64, 0, 321, "v3", 8, True),         # 321 = 5 * 64 + 1
    (64, 0, 640, "v3", 8, False),
    (64, 0, 590, "v3", 8, True),
    (64, 0, 334, "v3", 8, True),
    (64, 0, 641, "streamed", 4, False),
    (64, 0, 1102, "streamed", 4, False),
    (64, 1, 66, "streamed", 4, False),
    (64, 2, 384, "kv2", 12, False),
    (64, 2, 385, "streamed", 4, False),
    (64, 2, 17, "kv2", 1, False),
    (64, 3, 384, "kv3", 8, False),
    (64, 3, 385, "streamed", 4, False),
    (64, 3, 66, "kv3", 2, False),
    (64, 4, 258, "v2", 4, False),        # v2 has no TK = 1 instantiation
    (64, 4, 640, "v2", 8, False),
    (64, 4, 641, "streamed", 4, False),
    (64, 10, 320, "v2_valu", 4, False),
    (64, 10, 321, "v2_valu", 8, False),
    (64, 10, 641, "streamed", 4, False),
    (64, 11, 48, "v2", 4, False),        # nqt = 3 < 4 waves
    (64, 11, 49, "v3", 4, False),
    (64, 11, 321, "v3", 8, True),        # nqt = 21 >= 8
    (64, 7, 66, "streamed", 4, False),   # the Dh 72 algos on Dh 64
    (64, 14, 258, "v3", 4, True),        # 14 on Dh 64 = automatic
    (72, 0, 8, "streamed", 4, False),    # round32(8) = 32 > 2 * round8(8) = 16
    (72, 0, 9, "h72", 4, False),
    (72, 0, 16, "h72", 4, False),
    (72, 0, 17, "h72", 4, False),
    (72, 0, 280, "h72", 4, False),       # (280 + 288) * 144 = 81792 <= 81920
    (72, 0, 258, "h72", 4, True),
    (72, 7, 258, "h72", 4, True),
    (72, 0, 281, "streamed", 4, False),  # (288 + 288) * 144 = 82944
    (72, 14, 48, "h72", 4, False),       # nqt = 3 < 4
    (72, 14, 49, "h72p", 4, False),
    (72, 14, 258, "h72p", 4, False),     # h72p has no TK = 1 instantiation
    (72, 14, 281, "streamed", 4, False),
    (72, 14, 8, "streamed", 4, False),
    (72, 4, 66, "streamed", 4, False),   # the Dh 64 algos on Dh 72
    (72, 11, 66, "streamed", 4, False),
    (72, 1, 66, "streamed", 4, False),
]
for Dh in (32, 96, 128):
    for algo in (0, 1, 2, 3, 4, 7, 10, 11, 14):
        for L in (1, 17, 66, 258, 1102):
            TABLE.append((Dh, algo, L, "streamed", 4, False))


def test_symbol_declared_and_exported(lib):
    with open(os.path.join(REPO, "include", "pdm.h")) as f:
        header = f.read()
    assert re.search(r"\bint\s+pdm_attention_plan\s*\(", header)
    assert hasattr(lib, "pdm_attention_plan")
    from panopticdiffusionmodels_amd import _lib
    names = re.findall(r"#define\s+PDM_ATTN_(\w+)\s+(\d+)", header)
    assert [n.lower() for n, _ in names] == list(_lib.ATTENTION_FAMILIES)
    assert [int(v) for _, v in names] == list(range(8))


@pytest.mark.parametrize("Dh,algo,L,family,waves,tail1", TABLE)
def test_plan_table(lib, Dh, algo, L, family, waves, tail1):
    p = plan(lib, L, Dh, algo)
    assert (p.family, p.waves, p.tail1, p.variant) == (family, waves, tail1, 0), p
    nbh = B * H
    if family == "streamed":
        nqb = ((L + 15) // 16 + 3) // 4
        assert (p.grid, p.lds_bytes) == (8 * nqb, 0), p     # B H = 6 padded to 8 block slots per query block
    elif family in ("h72", "h72p"):
        assert (p.grid, p.lds_bytes) == (nbh, (r(L, 8) + r(L, 16)) * 144), p
    else:
        assert (p.grid, p.lds_bytes) == (nbh, r(L, 32) * 256), p


@pytest.mark.parametrize("algo,L,Dh,family,waves,variant", [
    (5, 258, 64, "v2", 4, 1), (6, 258, 64, "v2", 4, 2), (5, 590, 64, "v2", 8, 1), (6, 590, 64, "v2", 8, 2),
    (8, 258, 72, "h72", 4, 1), (9, 258, 72, "h72", 4, 2),
    (12, 258, 64, "v3", 4, 1), (13, 258, 64, "v3", 4, 2), (12, 590, 64, "v3", 8, 1), (13, 590, 64, "v3", 8, 2),
    (15, 258, 72, "h72p", 4, 1), (16, 258, 72, "h72p", 4, 2),
    (12, 48, 64, "v2", 4, 0),      # too few tiles for v3: the real v2
    (15, 48, 72, "h72", 4, 0),     # too few tiles for h72p: the real h72
    (15, 258, 64, "v3", 4, 0),     # 14-16 on Dh 64: automatic
    (5, 641, 64, "streamed", 4, 0), (8, 281, 72, "streamed", 4, 0),
])
def test_timing_variants_are_reported_and_never_tail1(lib, algo, L, Dh, family, waves, variant):
    p = plan(lib, L, Dh, algo)
    assert (p.family, p.waves, p.variant) == (family, waves, variant), p
    assert p.tail1 == (variant == 0 and family in ("v3", "h72") and L in (258, 590)), p


def _dispatcher_before(B, L, H, Dh, algo, ncu):
    """attention_launch as it was before the plan query, statement by statement (its launches as tuples)."""
    tail1 = L > 64 and L % 64 != 0 and L % 64 <= 16
    nqt, nbh = (L + 15) // 16, B * H
    Lp = r(L, 32)
    LV, L16 = r(L, 8), r(L, 16)
    smem72 = (LV + L16) * 144
    if Dh == 72 and smem72 <= 80 * 1024 and Lp <= 2 * LV and 14 <= algo <= 16 and nqt >= 4:
        return ("h72p", 4, False, algo - 14, min(nbh, 2 * ncu), smem72)
    if 14 <= algo <= 16:
        algo = 7 if Dh == 72 else 0
    if Dh == 72 and smem72 <= 80 * 1024 and Lp <= 2 * LV and (algo == 0 or 7 <= algo <= 9):
        if algo == 8:
            return ("h72", 4, False, 1, nbh, smem72)
        if algo == 9:
            return ("h72", 4, False, 2, nbh, smem72)
        return ("h72", 4, tail1, 0, nbh, smem72)
    if algo == 0 and Dh == 64 and Lp * 256 <= 160 * 1024:
        algo = 11
    if 11 <= algo <= 13 and Dh == 64 and Lp * 256 <= 160 * 1024:
        smem = Lp * 256
        nw = 4 if smem <= 80 * 1024 else 8
        if nqt >= nw:
            return ("v3", nw, algo == 11 and tail1, algo - 11, min(nbh, ncu * (2 if nw == 4 else 1)), smem)
        algo = 4
    if Dh != 64 or Lp * 256 > 160 * 1024:
        algo = 1
    if algo == 0 and Dh == 64 and Lp * 256 <= 160 * 1024:
        algo = 4
    if algo == 10 and Dh == 64 and Lp * 256 <= 160 * 1024:
        return ("v2_valu", 4 if Lp * 256 <= 80 * 1024 else 8, False, 0, nbh, Lp * 256)
    if 4 <= algo <= 6 and Dh == 64 and Lp * 256 <= 160 * 1024:
        return ("v2", 4 if Lp * 256 <= 80 * 1024 else 8, False, algo - 4, nbh, Lp * 256)
    if algo == 0 or algo >= 4:
        algo = 1
    if algo in (2, 3):
        nw = (nqt + algo - 1) // algo
        if nw <= (12 if algo == 2 else 8):
            return ("kv%d" % algo, nw, False, 0, nbh, Lp * 256)
    return ("streamed", 4, False, 0, (nbh + 7) // 8 * 8 * ((nqt + 3) // 4), 0)


@pytest.mark.parametrize("Dh", [32, 64, 72, 96, 128])
def test_every_shape_keeps_its_kernel(lib, Dh):
    """Exhaustive over L = 1 .. 700 (past every threshold) and a few long ones, every algo, two batch sizes and two
    CU counts: the plan equals what the dispatcher launched before it existed."""
    out = (ctypes.c_int * 6)()
    from panopticdiffusionmodels_amd._lib import ATTENTION_FAMILIES as FAM
    for algo in range(17):
        for L in list(range(1, 701)) + [1025, 1026, 1102, 2126, 4096]:
            for nb, nh, ncu in ((2, 3, 256), (75, 8, 304)):
                assert lib.pdm_attention_plan(nb, L, nh, Dh, algo, ncu, out) == OK
                got = (FAM[out[0]], out[1], bool(out[2]), out[3], out[4], out[5])
                assert got == _dispatcher_before(nb, L, nh, Dh, algo, ncu), (Dh, algo, L, nb, nh, ncu)


def test_persistent_grids(lib):
    for ncu in (256, 304, 8):
        for nbh in (1, 6, 2 * ncu - 1, 2 * ncu, 2 * ncu + 1, 600, 4800):
            assert plan(lib, 66, 64, 0, B=nbh, H=1, ncu=ncu).grid == min(nbh, 2 * ncu)        # v3, 4 waves
            assert plan(lib, 321, 64, 0, B=1, H=nbh, ncu=ncu).grid == min(nbh, ncu)           # v3, 8 waves
            assert plan(lib, 66, 72, 14, B=nbh, H=1, ncu=ncu).grid == min(nbh, 2 * ncu)       # h72p
            # one workgroup per head, whatever the device
            assert plan(lib, 66, 64, 4, B=nbh, H=1, ncu=ncu).grid == nbh
            assert plan(lib, 66, 64, 10, B=nbh, H=1, ncu=ncu).grid == nbh
            assert plan(lib, 66, 64, 2, B=nbh, H=1, ncu=ncu).grid == nbh
            assert plan(lib, 66, 72, 0, B=nbh, H=1, ncu=ncu).grid == nbh
    # the streamed kernel pads B H to a multiple of 8 block slots per query block (one XCD per head)
    for nbh, L, want in ((6, 66, 8 * 2), (8, 66, 8 * 2), (9, 66, 16 * 2), (9, 1102, 16 * 18), (1, 1, 8)):
        assert plan(lib, L, 96, 0, B=nbh, H=1).grid == want
    # ncu = 0 is the launcher's default, 256
    out = (ctypes.c_int * 6)()
    assert lib.pdm_attention_plan(600, 66, 1, 64, 0, 0, out) == OK and out[4] == 512


def test_plan_is_pure(lib):
    """Neither reads nor changes the global of pdm_set_attention_algo."""
    try:
        before = plan(lib, 258, 64)
        assert lib.pdm_set_attention_algo(1) == OK
        assert plan(lib, 258, 64) == before and before.family == "v3"
        assert plan(lib, 258, 64, 4).family == "v2"
        assert lib.pdm_set_attention_algo(0) == OK
        assert plan(lib, 258, 64, 1).family == "streamed"
    finally:
        lib.pdm_set_attention_algo(0)


def test_bad_arguments(lib):
    out = (ctypes.c_int * 6)()
    assert lib.pdm_attention_plan(2, 66, 3, 64, 0, 256, None) == ARG
    assert lib.pdm_attention_plan(2, 66, 3, 48, 0, 256, out) == ARG and b"head dim" in lib.pdm_last_error()
    for bad in ((0, 66, 3), (2, 0, 3), (2, 66, 0)):
        assert lib.pdm_attention_plan(*bad, 64, 0, 256, out) == ARG
    assert lib.pdm_attention_plan(2, 66, 3, 64, 17, 256, out) == ARG
    assert lib.pdm_attention_plan(2, 66, 3, 64, -1, 256, out) == ARG
    assert lib.pdm_attention_plan(2, 66, 3, 64, 0, -1, out) == ARG
    from panopticdiffusionmodels_amd import _lib
    with pytest.raises(ValueError):
        _lib.attention_plan(2, 66, 3, 40)
