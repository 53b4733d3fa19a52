"""The streaming attention backward (train_kernels.hip: attn_bwd_pre / dkv / dq kernels, any L, head dims 64 / 72)
through pdm_attention_backward_ex, against float64 autograd.

Bounds.  rel-L2 < 1e-2 per dq / dk / dv part is the project's bound for this kernel (tests/test_gpu_train.py).  A CPU
emulation of the kernel's rounding (o, P and dS rounded to bf16 once, fp32 accumulation: `emulate` below) gives
2.3e-3 - 2.8e-3 at every shape here, with no dependence on L, so the bound has about 4x headroom.  The spiky case's
bound is 2e-2; `test_spiky_reference_inside_its_bound` checks without a GPU that the emulation stays inside it.

Every call here writes into a dqkv buffer with 64 sentinel rows behind it and uses a scratch pre-filled with NaN:
the kernels may write nothing past a sequence and may not rely on the scratch's contents."""
import ctypes
import functools

import pytest
import torch

DEV = "cuda"
gpu = pytest.mark.gpu
SENTINEL = -1.2345e3


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _heads(x, B, L, n, H, Dh):
    return x.reshape(B, L, n, H, Dh).permute(2, 0, 3, 1, 4)


def _inputs(B, L, H, Dh, seed, spiky=False):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B * L, 3 * H * Dh, generator=g) * 1.5
    dout = torch.randn(B * L, H * Dh, generator=g).bfloat16()
    if spiky:   # one query row scaled by 8; key L // 3 dominates through a component every query shares (see SPIKY)
        v = qkv.reshape(B, L, 3, H, Dh)
        v[:, :, 0, :, 0] = v[:, :, 0, :, 0].abs() + 5.0
        v[:, L // 3, 1, :, 0] = 16.0
        v[:, L // 2, 0] *= 8.0
    return qkv.bfloat16(), dout


@functools.lru_cache(maxsize=None)
def case(B, L, H, Dh, spiky=False):
    """(qkv, dout, float64 autograd reference of dqkv), computed once per shape and shared"""
    qkv, dout = _inputs(B, L, H, Dh, B * 1000 + L + H + Dh, spiky)
    q = _heads(qkv.double(), B, L, 3, H, Dh).clone().requires_grad_(True)
    att = torch.softmax(q[0] @ q[1].transpose(-1, -2) * Dh ** -0.5, -1) @ q[2]
    att.permute(0, 2, 1, 3).reshape(B * L, H * Dh).backward(dout.double())
    ref = q.grad.permute(1, 3, 0, 2, 4).reshape(B * L, 3 * H * Dh)
    return qkv, dout, ref


def emulate(qkv, dout, B, L, H, Dh):
    """The kernels' arithmetic on the CPU: fp32 products and sums, o, P and dS rounded to bf16 once."""
    bf = lambda x: x.bfloat16().float()
    q, k, v = _heads(qkv.float(), B, L, 3, H, Dh)
    do = _heads(dout.float(), B, L, 1, H, Dh)[0]
    sc = Dh ** -0.5
    s = q @ k.transpose(-1, -2) * sc
    p = torch.exp(s - torch.logsumexp(s, -1, keepdim=True))
    o = bf(p @ v)
    delta = (do * o).sum(-1, keepdim=True)
    ds = bf(p * (do @ v.transpose(-1, -2) - delta))
    dv = bf(p).transpose(-1, -2) @ do
    dk = ds.transpose(-1, -2) @ q * sc
    dq = ds @ k * sc
    out = torch.stack([dq, dk, dv]).permute(1, 3, 0, 2, 4).reshape(B * L, 3 * H * Dh)
    return bf(out)


def run(qkv, dout, B, L, H, Dh, algo, o=None):
    """dqkv [B*L, 3*H*Dh] on the GPU; asserts the 64 rows behind it keep their bits"""
    from panopticdiffusionmodels_amd import _lib
    qkv, dout = qkv.to(DEV), dout.to(DEV)
    if o is None:
        o = _lib.attention(qkv, B, L, H, Dh)
    buf = torch.full((B * L + 64, 3 * H * Dh), SENTINEL, dtype=torch.bfloat16, device=DEV)
    want = buf[B * L:].clone()
    nbytes = ctypes.c_size_t(0)
    _lib.check(_lib.load().pdm_attention_backward_scratch_size(B, L, H, Dh, ctypes.byref(nbytes)))
    scratch = torch.full((nbytes.value // 4,), float("nan"), dtype=torch.float32, device=DEV)
    _lib.attention_backward(qkv, o, dout, B, L, H, Dh, algo=algo, out=buf, scratch=scratch)
    assert torch.equal(buf[B * L:].view(torch.int16), want.view(torch.int16)), "rows behind dqkv were written"
    return buf[:B * L], o


def parts(H, Dh):
    D = H * Dh
    return (("q", slice(0, D)), ("k", slice(D, 2 * D)), ("v", slice(2 * D, 3 * D)))


AUTO = [(64, 1, 609, 1), (64, 1, 640, 1), (64, 2, 641, 1), (64, 1, 1023, 1), (64, 2, 1102, 2), (64, 1, 2126, 2),
        (72, 1, 416, 1), (72, 2, 1026, 1), (72, 1, 1102, 2)]
FORCED = [(64, 3, 17, 2), (64, 2, 66, 1), (64, 2, 258, 2), (64, 2, 590, 2), (72, 2, 130, 1), (72, 2, 258, 2)]


@gpu
@pytest.mark.parametrize("Dh,B,L,H,algo", [c + (0,) for c in AUTO] + [c + (2,) for c in FORCED])
def test_stream_backward_vs_float64_autograd(Dh, B, L, H, algo):
    qkv, dout, ref = case(B, L, H, Dh)
    got, _ = run(qkv, dout, B, L, H, Dh, algo)
    assert bool(torch.isfinite(got.float()).all())
    errs = {name: rel(got[:, sl].float(), ref[:, sl]) for name, sl in parts(H, Dh)}
    print("rel-L2", (Dh, B, L, H, algo), errs)
    for name, e in errs.items():
        assert e < 1e-2, (name, e)


@gpu
@pytest.mark.parametrize("L", [641, 1102])
def test_sequences_are_isolated_at_ragged_tails(L):
    """B = 2: each sequence's dqkv has the bits of that sequence run alone (nothing crosses a sequence boundary in
    the tail tiles of the streamed operand or of the 128-row blocks)."""
    B, H, Dh = 2, 1, 64
    qkv, dout, _ = case(B, L, H, Dh)
    both, o = run(qkv, dout, B, L, H, Dh, 0)
    for b in range(B):
        sl = slice(b * L, (b + 1) * L)
        alone, _ = run(qkv[sl], dout[sl], 1, L, H, Dh, 0, o=o[sl].contiguous())
        assert torch.equal(alone.view(torch.int16), both[sl].view(torch.int16)), b


@gpu
def test_untouched_memory_and_nan_scratch():
    """`run` checks the sentinel rows on every call; here also that a NaN-filled scratch of exactly the advertised
    size gives a finite result at a length whose last block is ragged in every kernel (1102 = 8 * 128 + 78)."""
    B, L, H, Dh = 2, 1102, 2, 64
    qkv, dout, ref = case(B, L, H, Dh)
    got, _ = run(qkv, dout, B, L, H, Dh, 0)
    assert bool(torch.isfinite(got.float()).all())
    assert rel(got.float(), ref) < 1e-2


@gpu
def test_stream_backward_repeatable():
    """No atomics and a fixed reduction order: the same bits on every call (as test_attention_backward_long_repeatable
    states for the two-at-a-time kernel)."""
    B, L, H, Dh = 2, 1102, 2, 64
    qkv, dout, _ = case(B, L, H, Dh)
    d1, o = run(qkv, dout, B, L, H, Dh, 0)
    d2, _ = run(qkv, dout, B, L, H, Dh, 0, o=o)
    assert torch.equal(d1.view(torch.int16), d2.view(torch.int16))


# The spiky case: query row L // 2 scaled by 8 (scores up to ~100), and key L // 3 given a component (16) along one
# that every query has at >= 5, which adds >= 10 to its score in every row: it is the largest key of more than 90 %
# of the rows with a median probability of 0.9.  Pushed further (offset 8, component 20: the largest key of every row,
# probability >= 0.94) dq and dk become the rounding noise of the bf16 o in delta -- the emulation itself is then 0.2
# away from float64 -- and the comparison says nothing, so the construction stops where the emulation (8.8e-3) keeps
# the 2e-2 bound meaningful.
SPIKY = (1, 1102, 2, 64)


def test_spiky_reference_inside_its_bound():
    """Without a GPU: the rounding emulation of the spiky case stays within 2e-2 of float64, so the GPU test's bound
    needs no widening."""
    B, L, H, Dh = SPIKY
    qkv, dout, ref = case(B, L, H, Dh, True)
    emu = emulate(qkv, dout, B, L, H, Dh)
    errs = {name: rel(emu[:, sl], ref[:, sl]) for name, sl in parts(H, Dh)}
    print("emulation rel-L2 (spiky)", errs)
    assert max(errs.values()) < 2e-2, errs
    # the construction does what it says
    q, k, _ = _heads(qkv.double(), B, L, 3, H, Dh)
    s = q @ k.transpose(-1, -2) * Dh ** -0.5
    p = torch.softmax(s, -1)
    assert float((p.argmax(-1) == L // 3).double().mean()) > 0.9 and float(p[..., L // 3].median()) > 0.8
    assert float(s[:, :, L // 2].abs().max()) > 60.0


@gpu
def test_spiky_scores():
    B, L, H, Dh = SPIKY
    qkv, dout, ref = case(B, L, H, Dh, True)
    got, _ = run(qkv, dout, B, L, H, Dh, 0)
    assert bool(torch.isfinite(got.float()).all())
    errs = {name: rel(got[:, sl].float(), ref[:, sl]) for name, sl in parts(H, Dh)}
    print("rel-L2 (spiky)", errs)
    for name, e in errs.items():
        assert e < 2e-2, (name, e)


@gpu
@pytest.mark.parametrize("Dh,L", [(64, 1102), (64, 2126), (72, 1026)])
def test_forward_attention_at_the_long_lengths(Dh, L):
    """Coverage of the key-streaming forward kernel at the lengths the trainer now reaches (per-kernel bf16 bound)."""
    from panopticdiffusionmodels_amd import _lib
    B, H = 1, 2
    qkv, _, _ = case(B, L, H, Dh)
    q, k, v = _heads(qkv.float(), B, L, 3, H, Dh)
    ref = torch.nn.functional.scaled_dot_product_attention(q, k, v).permute(0, 2, 1, 3).reshape(B * L, H * Dh)
    out = _lib.attention(qkv.to(DEV), B, L, H, Dh)
    assert rel(out.float(), ref) <= 1e-2
