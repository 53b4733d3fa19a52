"""The forward attention kernels (csrc/attention.hip), every family the dispatcher can reach, through pdm_attention /
pdm_attention_log2 against float64 softmax attention on the CPU, per (query row, head).

Metrics, both against float64 computed from the bf16 inputs the kernel sees:
  (a) the worst relative L2 error over the (row, head) slices of Dh outputs;
  (b) the global relative L2 error.
Bounds on the GPU: (a) < 1e-2, (b) < 5e-3, twice what `emulate` (the kernels' rounding on the CPU: fp32 scores in log2
units, P = exp2(s - m) rounded to bf16 with m up to RESCALE_THR below the row maximum, fp32 accumulation, bf16 output)
reaches on the matrix of `test_emulation_is_inside_half_the_gpu_bounds`: (a) <= 5e-3, (b) <= 2.5e-3 (one mode has
bounds of its own, EMU_ROW_QROUND below).  `test_checker_rejects_known_defects` applies known defects to the
emulation and prints which of them the old test (one global rel-L2 < 1e-2, tests/test_gpu_kernels.py::test_attention*)
lets through: those confined to a key or a row, more of them the larger the shape.

With q_log2 the test pre-scales q by Dh^-0.5 log2(e) and rounds it to bf16, and the reference divides that rounded q
back in float64, so the comparison sees the kernel's error only.

`run` is the only way to the GPU here.  It asks pdm_attention_plan which kernel the shape and algo select and fails if
that is not the family the case names (a shape that falls back is a test error, not a silent pass); it never launches
a timing variant; qkv lies inside a NaN-filled allocation (64 rows before and behind, and the gap columns of a strided
case); the output lies inside a sentinel-filled one whose every element outside the live region must keep its bits,
and whose live region is pre-filled with a second sentinel that must not survive."""
import functools
import math

import pytest
import torch

DEV = "cuda"
gpu = pytest.mark.gpu
SENTINEL = -1.2345e3     # around the output
UNWRITTEN = 3.0e38       # in the output before the call (no attention output is that large)
PAD = 64                 # guard rows on each side
LOG2E = 1.4426950408889634
RESCALE_THR = 8.0
BOUND_ROW, BOUND_ALL = 1e-2, 5e-3            # GPU: twice ...
EMU_ROW, EMU_ALL = 5e-3, 2.5e-3              # ... what the emulation is held to
# The head-resident kernels without q_log2 multiply q by Dh^-0.5 log2(e) themselves and round the product to bf16 (the
# MFMA operand): one more rounding, of relative size 2^-9 on scores that reach +-100 in log2 units under the ramp and
# the spike, which the float64 reference does not share.  The emulation with that step reaches (a) 6.3e-2 / (b) 6.0e-3
# on the same matrix (plain inputs: 1.5e-2 / 3.8e-3), so this one mode has bounds of its own, again twice the
# emulation's.  It is a production mode: the trainer's forward (csrc/train.hip block_fwd) calls the kernels with
# q_log2 = 0 on the unscaled attn.qkv weights; only the inference forwards pack q pre-scaled.  The step has the size
# of the rounding the qkv GEMM already applied to q when it wrote bf16 (which the reference here takes as exact), so
# q carries two bf16 roundings there instead of one (attention section).  What holds the mode tight is
# test_unscaled_q_is_the_prescaled_kernel_after_one_rounding: bit equality with the q_log2 path, which is held to the
# bounds above.
EMU_ROW_QROUND, EMU_ALL_QROUND = 6.5e-2, 6.5e-3
RESIDENT = ("v2", "v2_valu", "v3", "h72", "h72p")
TIMING_ALGOS = (5, 6, 8, 9, 12, 13, 15, 16)  # wrong results by design: never launched
INPUTS = ("plain", "ramp", "spike", "last")


def _heads(x, B, L, n, H, Dh):
    return x.reshape(B, L, n, H, Dh).permute(2, 0, 3, 1, 4)


def _rows(o, B, L, H, Dh):
    return o.permute(0, 2, 1, 3).reshape(B * L, H * Dh)


def make_qkv(B, L, H, Dh, kind="plain", q_log2=False):
    """bf16 [B*L, 3*H*Dh], randn * 1.5.  ramp: keys grow x6 along the sequence; spike: key 3L/4 x8; last: the last
    key x6.  q_log2: q times Dh^-0.5 log2(e), rounded to bf16 (what the U-ViT qkv GEMM hands the kernels)."""
    g = torch.Generator().manual_seed(1000 * Dh + 10 * L + B + H + 7919 * INPUTS.index(kind))
    x = (torch.randn(B, L, 3, H, Dh, generator=g) * 1.5)
    if kind == "ramp":
        x[:, :, 1] *= torch.linspace(1.0, 6.0, L).reshape(1, L, 1, 1)
    elif kind == "spike":
        x[:, 3 * L // 4, 1] *= 8.0
    elif kind == "last":
        x[:, L - 1, 1] *= 6.0
    if q_log2:
        x[:, :, 0] *= Dh ** -0.5 * LOG2E
    return x.reshape(B * L, 3 * H * Dh).bfloat16()


def reference(qkv, B, L, H, Dh, q_log2):
    """float64 softmax attention from the bf16 qkv, [B*L, H*Dh]; a batch at a time (memory)."""
    out = torch.empty(B, H, L, Dh, dtype=torch.float64)
    x = qkv.reshape(B, L, 3, H, Dh)
    for b in range(B):
        q, k, v = x[b].double().permute(1, 2, 0, 3)
        if q_log2:
            q = q / (Dh ** -0.5 * LOG2E)
        out[b] = torch.softmax(q @ k.transpose(-1, -2) * Dh ** -0.5, -1) @ v
    return _rows(out, B, L, H, Dh)


@functools.lru_cache(maxsize=None)
def case(B, L, H, Dh, kind="plain", q_log2=False):
    """(qkv, float64 reference), computed once per case and shared; neither is ever modified"""
    qkv = make_qkv(B, L, H, Dh, kind, q_log2)
    return qkv, reference(qkv, B, L, H, Dh, q_log2)


def metrics(out, ref, H, Dh):
    """(a) worst relative L2 over (row, head) slices, (b) global relative L2"""
    o = torch.as_tensor(out).double().cpu().reshape(-1, H, Dh)
    r = ref.reshape(-1, H, Dh)
    a = float(((o - r).norm(dim=-1) / r.norm(dim=-1)).max())
    b = float((o - r).norm() / r.norm())
    return a, b


def within(ab, row=BOUND_ROW, total=BOUND_ALL):
    return ab[0] < row and ab[1] < total


def emulate(qkv, B, L, H, Dh, q_log2, resident=True, ones_sum=None, drop_key=None, skip_last_rescale=False,
            scale_twice=False):
    """The kernels' arithmetic on the CPU.  Scores are fp32 in log2 units; keys go by in blocks of 64 with a running
    maximum m; P = exp2(s - m) is rounded to bf16 for the P V product, which accumulates in fp32; the result is
    divided by the row sum and rounded to bf16.
    resident (v2 / v2_valu / v3 / h72 / h72p): m starts as block 0's maximum and moves only when a block exceeds it by
      more than RESCALE_THR (so it ends up to 8 below the true maximum and P reaches 2^8); without q_log2 the kernel
      scales q itself and rounds it to bf16 once more.
    not resident (streamed / kv2 / kv3): m is the true running maximum; without q_log2 the scale multiplies the fp32
      scores.
    ones_sum (default: resident; v2_valu: False): the row sum is taken from the bf16-rounded P (the ones-row MFMA),
      otherwise from the unrounded fp32 P (VALU adds).
    The three defects of test_checker_rejects_known_defects that live inside the loop: drop_key = (b, h, key) masks
    one key of one head; skip_last_rescale leaves the accumulator and the row sum unscaled when the last block moves
    m; scale_twice applies Dh^-0.5 log2(e) to pre-scaled scores again."""
    bf = lambda t: t.bfloat16().float()
    ones_sum = resident if ones_sum is None else ones_sum
    q, k, v = _heads(qkv.float(), B, L, 3, H, Dh)
    sl2 = torch.tensor(Dh ** -0.5, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
    if not q_log2 and resident:
        q = bf(q * sl2)
    s = q @ k.transpose(-1, -2)
    if (not q_log2 and not resident) or scale_twice:
        s = s * sl2
    if drop_key is not None:
        s[drop_key[0], drop_key[1], :, drop_key[2]] = -math.inf
    thr = RESCALE_THR if resident else 0.0
    m = s[..., :64].max(-1, keepdim=True).values
    acc = torch.zeros(B, H, L, Dh)
    lsum = torch.zeros(B, H, L, 1)
    nblk = (L + 63) // 64
    for c in range(nblk):
        sb = s[..., c * 64:(c + 1) * 64] - m
        if c > 0:
            over = sb.max(-1, keepdim=True).values
            d = torch.where(over > thr, over, torch.zeros_like(over))
            m = m + d
            sb = sb - d
            if not (skip_last_rescale and c == nblk - 1):
                alpha = torch.exp2(-d)
                acc, lsum = acc * alpha, lsum * alpha
        p = torch.exp2(sb)
        lsum = lsum + (bf(p) if ones_sum else p).sum(-1, keepdim=True)
        acc = acc + bf(p) @ v[..., c * 64:(c + 1) * 64, :]
    return _rows(bf(acc / lsum), B, L, H, Dh)


def bounds(family, q_log2):
    """GPU bounds (a), (b) of a kernel family: twice the emulation's"""
    if family in RESIDENT and not q_log2:
        return 2 * EMU_ROW_QROUND, 2 * EMU_ALL_QROUND
    return BOUND_ROW, BOUND_ALL


# ---- without a GPU: the emulation justifies the bounds, and the checker has teeth -------------------------------

@pytest.mark.parametrize("L", [1, 5, 17, 66, 258, 590, 1102])
def test_emulation_is_inside_half_the_gpu_bounds(L):
    """Dh {32, 64, 72, 128} x every input family at B = 2, H = 3, in every mode a kernel of that head dim has (the
    streamed kernel at every Dh; the head-resident ones, with either kind of row sum, at 64 and 72): (a) <= 5e-3 and
    (b) <= 2.5e-3 -- for the head-resident kernels' own scaling of q, which rounds q once more, 6.5e-2 and 6.5e-3 --
    and no reference slice is near zero, so the per-row relative metric is well defined."""
    B, H = 2, 3
    worst = {}
    for Dh in (32, 64, 72, 128):
        modes = [("streamed", dict(resident=False))]
        if Dh in (64, 72):
            modes += [("resident", dict(resident=True)), ("resident, VALU sums", dict(resident=True, ones_sum=False))]
        for kind in INPUTS:
            for q_log2 in (True, False):
                qkv, ref = case(B, L, H, Dh, kind, q_log2)
                assert float(ref.reshape(-1, H, Dh).norm(dim=-1).min()) > 0.25
                for name, kw in modes:
                    ab = metrics(emulate(qkv, B, L, H, Dh, q_log2, **kw), ref, H, Dh)
                    qround = kw["resident"] and not q_log2
                    key = (name, "q rounded in the kernel" if qround else "q_log2" if q_log2 else "fp32 scale")
                    worst[key] = tuple(max(x, y) for x, y in zip(worst.get(key, (0.0, 0.0)), ab))
                    lim = (EMU_ROW_QROUND, EMU_ALL_QROUND) if qround else (EMU_ROW, EMU_ALL)
                    assert ab[0] <= lim[0] and ab[1] <= lim[1], (Dh, kind, q_log2, name, ab)
    for key, ab in sorted(worst.items()):
        print("emulation L=%d %s, %s: worst (a) %.2e (b) %.2e" % ((L,) + key + ab))


def test_checker_rejects_known_defects():
    """Known defects applied to the emulation's output (Dh 64, q_log2), at this file's shape (B 2, H 3, L 258 / 256)
    and at one of the old test's (tests/test_gpu_kernels.py::test_attention_algos: B 3, H 4, L 334 / 320): each must
    fail (a) < 1e-2 or (b) < 5e-3.  Printed: which of them the old check, one global rel-L2 < 1e-2, lets through.  A
    defect confined to one row or one key moves the global figure by its size / sqrt(rows), so the old check loses
    it as the shape grows; (a) does not depend on the shape."""
    Dh = 64
    passed_old = []
    for B, H, L in ((2, 3, 258), (3, 4, 334)):
        def emu(L, kind, **kw):
            qkv, ref = case(B, L, H, Dh, kind, True)
            return emulate(qkv, B, L, H, Dh, True, **kw), ref

        good, ref = emu(L, "plain")
        assert within(metrics(good, ref, H, Dh))
        defects = {}
        # one key dropped from the last ragged block of one head
        defects["last key of head (1, 2) dropped"] = (emu(L, "plain", drop_key=(1, 2, L - 1))[0], ref)
        # two adjacent query rows of one head swapped
        o = good.clone()
        o[[100, 101], Dh:2 * Dh] = good[[101, 100], Dh:2 * Dh]
        defects["query rows 100 / 101 of head (0, 1) swapped"] = (o, ref)
        # one head's output written at the neighbouring head's columns (its own left unwritten: zero)
        o = good.clone()
        o[L:2 * L, 2 * Dh:3 * Dh] = good[L:2 * L, Dh:2 * Dh]
        o[L:2 * L, Dh:2 * Dh] = 0
        defects["head (1, 1) written at head (1, 2)'s columns"] = (o, ref)
        # the rescale of the accumulator skipped when the last 64-key block moves the running max (ramp)
        Lr = L // 64 * 64
        goodr, refr = emu(Lr, "ramp")
        assert within(metrics(goodr, refr, H, Dh))
        bad = emu(Lr, "ramp", skip_last_rescale=True)[0]
        assert not torch.equal(bad, goodr)
        defects["rescale skipped in the last 64-key block (ramp)"] = (bad, refr)
        # the q_log2 scale applied twice
        defects["q_log2 scale applied twice"] = (emu(L, "plain", scale_twice=True)[0], ref)
        for name, (o, r) in defects.items():
            ab = metrics(o, r, H, Dh)
            old = ab[1] < 1e-2
            print("B %d H %d L %d  %-48s (a) %.2e (b) %.2e  this check: %s, the old global 1e-2: %s"
                  % (B, H, L, name, ab[0], ab[1], "PASSES" if within(ab) else "rejects",
                     "passes" if old else "rejects"))
            assert not within(ab), (name, ab)
            if old:
                passed_old.append((name, (B, H, L)))
    print("defects the old global 1e-2 bound lets through:", passed_old)


# ---- on the GPU ----------------------------------------------------------------------------------------------------

def _ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def run(qkv, B, L, H, Dh, algo, family, q_log2, strided=False):
    """The output [B*L, H*Dh] (CPU) of the kernel `family` that `algo` selects for this shape; see the module
    docstring for what it asserts on the way."""
    from panopticdiffusionmodels_amd import _lib
    assert algo not in TIMING_ALGOS, algo
    plan = _lib.attention_plan(B, L, H, Dh, algo, _ncu())
    assert plan.family == family and plan.variant == 0, (plan, "wanted " + family)
    D, rows = H * Dh, B * L
    ldq, ldo = 3 * D + (8 if strided else 0), D + (4 if strided else 0)
    qbuf = torch.full((rows + 2 * PAD, ldq), float("nan"), dtype=torch.bfloat16, device=DEV)
    qbuf[PAD:PAD + rows, :3 * D] = qkv.to(DEV)
    obuf = torch.full((rows + 2 * PAD, ldo), SENTINEL, dtype=torch.bfloat16, device=DEV)
    obuf[PAD:PAD + rows, :D] = UNWRITTEN
    want = obuf.clone()
    qv, ov = qbuf[PAD:PAD + rows, :3 * D], obuf[PAD:PAD + rows, :D]
    assert qv.stride(0) == ldq and ov.stride(0) == ldo
    _lib.check(_lib.load().pdm_set_attention_algo(algo), "pdm_set_attention_algo")
    try:
        ret = _lib.attention(qv, B, L, H, Dh, q_log2=q_log2, out=ov)
        torch.cuda.synchronize()
    finally:
        _lib.load().pdm_set_attention_algo(0)
    assert ret.data_ptr() == ov.data_ptr()
    out = ov.clone()
    assert not bool((out.view(torch.int16) == want[PAD:PAD + rows, :D].view(torch.int16)).any()), \
        "part of the output was not written"
    assert bool(torch.isfinite(out.float()).all()), "non-finite output"
    want[PAD:PAD + rows, :D] = out
    assert torch.equal(obuf.view(torch.int16), want.view(torch.int16)), "memory outside the output rows was written"
    return out.cpu(), plan


def kinds(L):
    """plain plus the stressing inputs of a length: the dominant last key where the last key block is ragged (else the
    spike), and the ramp wherever there is more than one key block"""
    return ("plain", "last" if L % 64 else "spike") + (("ramp",) if L > 64 else ())


def check(family, Dh, algo, L, B=2, H=3, strided=False, which=None, log2=(True, False)):
    """every input family of this L x q_log2 {1, 0}: (a) and (b) against float64, printed, then asserted"""
    bad, worst = [], {}
    for kind in which or kinds(L):
        for q_log2 in log2:
            qkv, ref = case(B, L, H, Dh, kind, q_log2)
            out, plan = run(qkv, B, L, H, Dh, algo, family, q_log2, strided)
            ab = metrics(out, ref, H, Dh)
            lim = bounds(family, q_log2)
            print("%-8s Dh %3d L %4d B %d H %d %s %-5s q_log2 %d  waves %2d tail1 %d grid %4d  (a) %.2e (b) %.2e"
                  "  bounds %.1e / %.1e" % (family, Dh, L, B, H, "strided" if strided else "dense  ", kind, q_log2,
                                            plan.waves, plan.tail1, plan.grid, ab[0], ab[1], lim[0], lim[1]))
            worst[lim] = tuple(max(x, y) for x, y in zip(worst.get(lim, (0.0, 0.0)), ab))
            if not within(ab, *lim):
                bad.append((kind, q_log2, ab, lim))
    for lim, ab in sorted(worst.items()):   # one line per set of bounds (q rounded in the kernel has its own)
        print("worst of %s Dh %d L %d under the bounds %.1e / %.1e: (a) %.2e (b) %.2e" % ((family, Dh, L) + lim + ab))
    assert not bad, bad


STREAMED = ([(Dh, 1 if Dh == 72 else 0, L) for Dh in (32, 72, 96, 128) for L in (1, 15, 16, 17, 63, 64, 65, 130)]
            + [(72, 0, 8), (72, 0, 281)]                           # the automatic choice on both sides of h72
            + [(64, 1, L) for L in (1, 17, 64, 65, 258)]
            + [(64, 0, 641), (64, 0, 1102)])                        # the automatic choice past the LDS-resident limit
V2_L = (1, 15, 16, 17, 48, 64, 65, 80, 81, 129, 257, 258, 320, 321, 513, 590, 640)
V3_L = (49, 64, 65, 80, 81, 258, 320, 321, 334, 590, 640)
KV_L = (17, 64, 66, 129, 258, 384)
H72_L = (9, 16, 17, 33, 64, 65, 80, 81, 258, 280)
H72P_L = (49, 66, 257, 258, 280)
# family -> (Dh, algo)
FORCED = {"kv2": (64, 2), "kv3": (64, 3), "v2": (64, 4), "v2_valu": (64, 10), "v3": (64, 11), "h72": (72, 7),
          "h72p": (72, 14)}


@gpu
@pytest.mark.parametrize("Dh,algo,L", STREAMED)
def test_streamed(Dh, algo, L):
    """B H = 6 is no multiple of 8: the padded grid has dead blocks"""
    check("streamed", Dh, algo, L)


@gpu
@pytest.mark.parametrize("B,H", [(2, 4), (3, 3)])
@pytest.mark.parametrize("Dh", [64, 96])
def test_streamed_full_and_spilling_block_groups(Dh, B, H):
    """B H = 8 fills one group of 8 block slots exactly, 9 spills one head into a second group"""
    check("streamed", Dh, 1, 130, B=B, H=H)


@gpu
@pytest.mark.parametrize("L", KV_L)
@pytest.mark.parametrize("family", ["kv2", "kv3"])
def test_kv(family, L):
    check(family, *FORCED[family], L)


@gpu
@pytest.mark.parametrize("L", V2_L)
@pytest.mark.parametrize("family", ["v2", "v2_valu"])
def test_v2(family, L):
    check(family, *FORCED[family], L)


@gpu
@pytest.mark.parametrize("L", V3_L)
def test_v3(L):
    check("v3", 64, 11, L)


@gpu
@pytest.mark.parametrize("L", [49, 258, 321, 590])
def test_v3_is_the_automatic_choice(L):
    check("v3", 64, 0, L, which=("plain",))


@gpu
@pytest.mark.parametrize("L", H72_L)
def test_h72(L):
    check("h72", 72, 7, L)


@gpu
@pytest.mark.parametrize("L", [9, 16, 258, 280])
def test_h72_is_the_automatic_choice(L):
    check("h72", 72, 0, L, which=("plain",))


@gpu
@pytest.mark.parametrize("L", H72P_L)
def test_h72p(L):
    check("h72p", 72, 14, L)


@gpu
@pytest.mark.parametrize("family,Dh,algo,L", [("streamed", 128, 0, 65), ("streamed", 72, 1, 130)]
                         + [(f,) + FORCED[f] + (258,) for f in FORCED])
def test_row_strides(family, Dh, algo, L):
    """ldq = 3 H Dh + 8 and ldo = H Dh + 4 (both inside attention_check's alignment rules): NaN in the gap columns of
    qkv, sentinels in the output's"""
    check(family, Dh, algo, L, strided=True)


def _prescaled(qkv, H, Dh):
    """q * (Dh^-0.5 * log2 e), product and factor in fp32, rounded to bf16: what the head-resident kernels make of an
    unscaled q"""
    sl2 = torch.tensor(Dh ** -0.5, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
    out = qkv.clone()
    out[:, :H * Dh] = (qkv[:, :H * Dh].float() * sl2).bfloat16()
    return out


@gpu
@pytest.mark.parametrize("family,L", [("v2", 17), ("v2", 258), ("v2", 590), ("v2_valu", 258), ("v2_valu", 590),
                                      ("v3", 66), ("v3", 258), ("v3", 590), ("h72", 16), ("h72", 258), ("h72", 280),
                                      ("h72p", 66), ("h72p", 258)])
def test_unscaled_q_is_the_prescaled_kernel_after_one_rounding(family, L):
    """The head-resident kernels read q_log2 themselves: without it they multiply q by Dh^-0.5 log2(e) and round to
    bf16, then run the same code.  So pdm_attention on q has the bits of pdm_attention_log2 on that rounded product,
    which ties the mode with the looser float64 bounds to the one with the tight ones."""
    B, H = 2, 3
    Dh, algo = FORCED[family]
    for kind in kinds(L):
        qkv, _ = case(B, L, H, Dh, kind, False)
        plain, _ = run(qkv, B, L, H, Dh, algo, family, False)
        pre, _ = run(_prescaled(qkv, H, Dh), B, L, H, Dh, algo, family, True)
        assert torch.equal(plain.view(torch.int16), pre.view(torch.int16)), kind


PERSISTENT = [("v3", 4, 200, 3, 66), ("v3", 8, 100, 3, 321), ("h72p", 4, 200, 3, 66)]


@gpu
@pytest.mark.parametrize("family,waves,B,H,L", PERSISTENT)
def test_persistent_kernels_over_several_heads(family, waves, B, H, L):
    """The smallest shapes at which a workgroup of the persistent kernels runs more than one head (B H = 600 > 2 CUs
    with 4 waves, 300 > CUs with 8): the per-row bound, the bits of the one-head-per-workgroup kernel (v2, h72), and
    the same bits on a second run."""
    Dh, algo = FORCED[family]
    one = "v2" if family == "v3" else "h72"
    for q_log2 in (True, False):
        qkv, ref = case(B, L, H, Dh, "ramp", q_log2)
        out, plan = run(qkv, B, L, H, Dh, algo, family, q_log2)
        assert plan.waves == waves and plan.grid < B * H, plan
        ab = metrics(out, ref, H, Dh)
        print("%s persistent B %d H %d L %d q_log2 %d grid %d: (a) %.2e (b) %.2e" % (family, B, H, L, q_log2, plan.grid,
                                                                                     ab[0], ab[1]))
        assert within(ab, *bounds(family, q_log2)), ab
        again, _ = run(qkv, B, L, H, Dh, algo, family, q_log2)
        assert torch.equal(out.view(torch.int16), again.view(torch.int16)), "two runs differ"
        single, _ = run(qkv, B, L, H, Dh, FORCED[one][1], one, q_log2)
        assert torch.equal(out.view(torch.int16), single.view(torch.int16)), "differs from " + one


@gpu
@pytest.mark.parametrize("family,Dh,algo,L", [("streamed", 96, 0, 130), ("streamed", 64, 0, 641)]
                         + [(f,) + FORCED[f] + (258,) for f in FORCED])
def test_sequences_are_isolated(family, Dh, algo, L):
    """B = 3 at a ragged L: every sequence has the bits of that sequence run alone"""
    B, H = 3, 3
    for q_log2 in (True, False):
        qkv, _ = case(B, L, H, Dh, "last", q_log2)
        both, _ = run(qkv, B, L, H, Dh, algo, family, q_log2)
        for b in range(B):
            sl = slice(b * L, (b + 1) * L)
            alone, _ = run(qkv[sl], 1, L, H, Dh, algo, family, q_log2)
            assert torch.equal(alone.view(torch.int16), both[sl].view(torch.int16)), (b, q_log2)
