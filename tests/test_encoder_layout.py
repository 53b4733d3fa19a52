"""Host-logic checks of the HIP encoder (no GPU): the `pdm_encoder_*` parameter table against `weights.encoder_spec`,
the spec's keys against the reference's own state_dict key list (tests/golden/encoder_golden.npz), the seeded decoder
weights staying what they were, and the downsample's gather + GEMM layout (csrc/decoder.hip down_gather_kernel:
A[pixel][(ky*3 + kx)*C + ci] = X[2y + ky][2x + kx][ci], zero at row H / column W) times the weight exactly as
`_EncoderHandle._pack` packs it against F.conv2d at stride 2 on the right/bottom-padded input."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from panopticdiffusionmodels_amd import _lib
from panopticdiffusionmodels_amd import weights as W
from panopticdiffusionmodels_amd.libs.autoencoder import FrozenAutoencoderKL, _EncoderHandle

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def enc_golden():
    return np.load(os.path.join(REPO, "tests", "golden", "encoder_golden.npz"))


def _cfg(ch, mult, nrb, latent, in_channels=3, z_channels=4, double_z=1):
    cfg = _lib.PdmEncoderCfg()
    cfg.ch = ch
    for i, m in enumerate(mult):
        cfg.ch_mult[i] = m
    cfg.num_levels = len(mult)
    cfg.num_res_blocks = nrb
    cfg.in_channels = in_channels
    cfg.z_channels = z_channels
    cfg.double_z = double_z
    cfg.latent_size = latent
    return cfg


def _table(lib, h):
    buf = ctypes.create_string_buffer(256)
    out = []
    for i in range(lib.pdm_encoder_param_count(h)):
        dt, ne = ctypes.c_int(), ctypes.c_longlong()
        _lib.check(lib.pdm_encoder_param_info(h, i, buf, 256, ctypes.byref(dt), ctypes.byref(ne)))
        out.append((buf.value.decode(), dt.value, ne.value))
    return out


@pytest.mark.parametrize("ch,mult,nrb,latent", [(64, (1, 2), 1, 24), (128, (1, 2, 4, 4), 2, 32),
                                                (128, (1, 2, 4, 4), 2, 64)])
def test_param_table_matches_spec_without_gpu(ch, mult, nrb, latent):
    lib = _lib.load()
    h = ctypes.c_void_p()
    _lib.check(lib.pdm_encoder_create(ctypes.byref(_cfg(ch, mult, nrb, latent)), ctypes.byref(h)))
    try:
        spec = W.encoder_spec(ch=ch, ch_mult=mult, num_res_blocks=nrb)
        shapes = {k: int(np.prod(s)) for k, s, _ in spec}
        table = _table(lib, h)
        seen = set()
        for name, dt, ne in table:
            if ".mid.attn_1.qkv." in name:   # q, k, v packed into one matrix / bias
                p, leaf = name.split("qkv.")
                assert ne == sum(shapes[f"{p}{n}.{leaf}"] for n in "qkv"), name
                seen.update(f"{p}{n}.{leaf}" for n in "qkv")
                continue
            assert name in shapes, name
            if name.startswith(("encoder.conv_out.", "quant_conv.")):   # may be padded
                assert ne >= shapes[name], name
            else:
                assert ne == shapes[name], name
            assert dt == (_lib.PDM_BF16 if name.endswith(".weight") and "norm" not in name and
                          name not in ("encoder.conv_in.weight", "quant_conv.weight") else _lib.PDM_F32), name
            seen.add(name)
        assert seen == set(shapes)   # every reference key is registered
        ws1, ws2 = ctypes.c_size_t(), ctypes.c_size_t()
        _lib.check(lib.pdm_encoder_workspace_size(h, 1, ctypes.byref(ws1)))
        _lib.check(lib.pdm_encoder_workspace_size(h, 2, ctypes.byref(ws2)))
        assert 0 < ws1.value < ws2.value
        # encoding without registered weights fails with the state error (no GPU call happens)
        st = lib.pdm_encoder_encode_moments(h, ctypes.c_void_p(16), ctypes.c_void_p(16), 1, ctypes.c_void_p(16),
                                            1 << 40, None)
        assert st == 3 and b"not registered" in lib.pdm_last_error()
    finally:
        lib.pdm_encoder_destroy(h)


@pytest.mark.parametrize("kw", [dict(ch=32), dict(ch=2048, mult=(1,)), dict(mult=(1, 2, 4, 4, 4)), dict(mult=()),
                                dict(in_channels=4), dict(z_channels=8), dict(double_z=0), dict(latent=5),
                                dict(latent=12), dict(latent=72), dict(mult=(1, 3), ch=96), dict(ch=64, mult=(1, 32))])
def test_create_rejects_unsupported(kw):
    lib = _lib.load()
    a = dict(ch=128, mult=(1, 2, 4, 4), nrb=2, latent=32)
    a.update(kw)
    cfg = _cfg(a["ch"], a["mult"][:4], a["nrb"], a["latent"], **{k: a[k] for k in a if k in
                                                                 ("in_channels", "z_channels", "double_z")})
    cfg.num_levels = len(a["mult"])
    h = ctypes.c_void_p()
    with pytest.raises(ValueError):
        _lib.check(lib.pdm_encoder_create(ctypes.byref(cfg), ctypes.byref(h)))


def test_spec_keys_match_reference_key_list(enc_golden):
    keys = [k for k, _, _ in W.encoder_spec()]
    assert keys == [str(k) for k in enc_golden["state_dict_keys"]]
    assert keys == [k for k, _, _ in W.encoder_spec(**W.ENCODER_DDCONFIG)]


def test_seeded_decoder_weights_unchanged(golden):
    a = W.decoder_state_dict(seed=1)
    b = W.make_state_dict(W.decoder_spec(), seed=1)
    assert list(a) == list(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    # the full decoder of golden.npz (seed 1, reference init): the checksum stored before the encoder existed
    chk = np.array([float(v.double().sum()) for v in a.values()] + [float(v.double().abs().sum()) for v in a.values()])
    # (fp64 sums: their last bits depend on the summation order, so the checksum tolerance of test_oracle_golden.py)
    np.testing.assert_allclose(chk, golden["decoder_full/sd_checksum"], rtol=1e-12, atol=1e-9)
    # and the encoder's weights come from their own generator: the same seed does not shift the decoder's
    e = W.encoder_state_dict(seed=1)
    assert not set(e) & set(a)
    ae = FrozenAutoencoderKL(seed=1)
    for k in a:
        assert torch.equal(ae._p(k), a[k]), k


def test_encoder_keys_all_or_none():
    dsd = W.make_state_dict(W.decoder_spec(ch=64, ch_mult=(1, 2), num_res_blocks=1), seed=7)
    esd = W.encoder_state_dict(seed=7, ch=64, ch_mult=(1, 2), num_res_blocks=1)
    dd = dict(W.DECODER_DDCONFIG, ch=64, ch_mult=[1, 2], num_res_blocks=1)
    full = dict(dsd, **esd)
    ae = FrozenAutoencoderKL(dd, 4, state_dict=full, latent_size=8)
    assert torch.equal(ae._p("encoder.conv_in.weight"), esd["encoder.conv_in.weight"])
    part = dict(full)
    del part["encoder.mid.attn_1.k.weight"], part["quant_conv.bias"]
    with pytest.raises(RuntimeError, match="encoder.mid.attn_1.k.weight"):
        FrozenAutoencoderKL(dd, 4, state_dict=part, latent_size=8)
    only_dec = FrozenAutoencoderKL(dd, 4, state_dict=dsd, latent_size=8)
    # decoder-only construction is what it always was: the decoder's buffers and nothing else
    assert list(only_dec.state_dict()) == [k.replace(".", "__") for k in dsd]
    assert list(FrozenAutoencoderKL(dd, 4, latent_size=8).state_dict()) == [k.replace(".", "__") for k in dsd]


def test_downsample_gather_layout_and_packing():
    """The gather kernel's documented layout, restated in torch, times the packed weight == Downsample.forward."""
    ch, mult, nrb = 64, (1, 2), 1
    esd = W.encoder_state_dict(seed=5, init="random", ch=ch, ch_mult=mult, num_res_blocks=nrb)
    esd = {k: v.bfloat16().float() for k, v in esd.items()}   # bf16-exact weights: the packing is lossless
    dsd = W.make_state_dict(W.decoder_spec(ch=ch, ch_mult=mult, num_res_blocks=nrb), seed=5)
    dd = dict(W.DECODER_DDCONFIG, ch=ch, ch_mult=list(mult), num_res_blocks=nrb)
    ae = FrozenAutoencoderKL(dd, 4, state_dict=dict(dsd, **esd), latent_size=8)
    name = "encoder.down.0.downsample.conv.weight"
    wp = _EncoderHandle._pack(ae, name, _lib.PDM_BF16)
    assert wp.dtype == torch.bfloat16 and tuple(wp.shape) == (ch, 9 * ch)
    bias = _EncoderHandle._pack(ae, "encoder.down.0.downsample.conv.bias", _lib.PDM_F32)
    B, H = 2, 6
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, ch, H, H, generator=g)
    xp = F.pad(x, (0, 1, 0, 1))                                  # libs/autoencoder.py:67-68
    cols = F.unfold(xp, kernel_size=3, stride=2)                 # [B, C*9, L], rows ordered (ci, ky, kx)
    L = cols.shape[-1]
    A = cols.reshape(B, ch, 3, 3, L).permute(0, 4, 2, 3, 1).reshape(B * L, 9 * ch)   # (ky, kx, ci) columns
    got = (A @ wp.float().t() + bias).reshape(B, H // 2, H // 2, ch).permute(0, 3, 1, 2)
    ref = F.conv2d(xp, esd[name], esd["encoder.down.0.downsample.conv.bias"], stride=2)
    assert got.shape == ref.shape
    assert float((got - ref).norm() / ref.norm()) < 1e-5
    # the gather's own index arithmetic (thread -> (pixel, tap, channel octet)) against the same matrix
    xn = x.permute(0, 2, 3, 1).contiguous()                      # NHWC
    A2 = torch.zeros(B * L, 9 * ch)
    Ho = H // 2
    for m in range(B * L):
        b, p = divmod(m, Ho * Ho)
        for tap in range(9):
            yy, xx = 2 * (p // Ho) + tap // 3, 2 * (p % Ho) + tap % 3
            if yy < H and xx < H:
                A2[m, tap * ch:(tap + 1) * ch] = xn[b, yy, xx]
    assert torch.equal(A2, A)
    # the other packed forms the encoder relies on
    co = _EncoderHandle._pack(ae, "encoder.conv_out.weight", _lib.PDM_BF16)
    assert tuple(co.shape) == (8, 9 * ch * mult[-1])
    assert torch.equal(co.float().reshape(8, 3, 3, -1), esd["encoder.conv_out.weight"].permute(0, 2, 3, 1))
    ci = _EncoderHandle._pack(ae, "encoder.conv_in.weight", _lib.PDM_F32)
    assert torch.equal(ci, esd["encoder.conv_in.weight"].reshape(-1))


def test_encode_refuses_cpu_and_decoder_only_weights():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    ae = FrozenAutoencoderKL()
    with pytest.raises(RuntimeError):
        ae.encode_moments(torch.zeros(1, 3, 64, 64))
    with pytest.raises(RuntimeError):
        ae.sample(torch.zeros(1, 8, 8, 8))
