"""HIP KL-f8 encoder (csrc/decoder.hip pdm_encoder_*) against the reference Encoder + quant_conv's own fp32 outputs
(tests/golden/encoder_golden.npz, made by tests/golden/make_encoder_golden.py from libs/autoencoder.py).  Tolerance on
the moments: rel-L2 < 2e-2, the project's bound for bf16 operands with fp32 accumulation and an fp32 residual stream
(tests/test_gpu_decoder.py); `sample` is elementwise fp32 and pinned at 1e-5.

Measured on the MI355X (rel-L2 of the moments vs the fixture): DESIGN.md §5a "Parity".
"""
import os

import numpy as np
import pytest
import torch

from panopticdiffusionmodels_amd import _lib
from panopticdiffusionmodels_amd import weights as W
from panopticdiffusionmodels_amd.libs import autoencoder as AE
from panopticdiffusionmodels_amd.libs.autoencoder import FrozenAutoencoderKL

pytestmark = pytest.mark.gpu
TOL = 2e-2
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# key -> ch, ch_mult, num_res_blocks, weight seed, init, batch, image side (the table of make_encoder_golden.py)
CASES = {
    "enc64": (64, (1, 2), 1, 31, "random", 3, 48),
    "enc_full128": (128, (1, 2, 4, 4), 2, 32, "reference", 1, 128),
    "enc_full256": (128, (1, 2, 4, 4), 2, 33, "random", 2, 256),
    "enc_full512": (128, (1, 2, 4, 4), 2, 34, "reference", 1, 512),
}


def rel(a, b):
    a = torch.as_tensor(a).double().cpu()
    b = torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(REPO, "tests", "golden", "encoder_golden.npz"))


def _images(seed, batch, side):
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.rand(batch, 3, side, side, generator=g) * 2.0 - 1.0


def _ae(ch, mult, nrb, seed, init, encoder=True, **kw):
    sd = W.make_state_dict(W.decoder_spec(ch=ch, ch_mult=mult, num_res_blocks=nrb), seed=seed, init=init)
    if encoder:
        sd.update(W.encoder_state_dict(seed=seed, init=init, ch=ch, ch_mult=mult, num_res_blocks=nrb))
    dd = dict(W.DECODER_DDCONFIG, ch=ch, ch_mult=list(mult), num_res_blocks=nrb)
    return FrozenAutoencoderKL(dd, 4, state_dict=sd, **kw)


def _case(fx, key):
    ch, mult, nrb, seed, init, batch, side = CASES[key]
    x = _images(seed, batch, side)
    sums = np.array([float(x[i].double().sum()) for i in range(batch)])
    np.testing.assert_allclose(sums, fx[f"{key}/img_sum"], rtol=0, atol=1e-6)   # the same images as the fixture's
    sd = W.encoder_state_dict(seed=seed, init=init, ch=ch, ch_mult=mult, num_res_blocks=nrb)
    chk = np.array([float(v.double().sum()) for v in sd.values()] + [float(v.double().abs().sum()) for v in sd.values()])
    np.testing.assert_allclose(chk, fx[f"{key}/sd_checksum"], rtol=1e-12, atol=1e-9)
    return _ae(ch, mult, nrb, seed, init), x


@pytest.mark.parametrize("key", ["enc64", "enc_full128", "enc_full512"])
def test_encode_moments_vs_reference_golden(fx, dev, key):
    ae, x = _case(fx, key)
    m = ae.to(dev).encode_moments(x.to(dev))
    ref = fx[f"{key}/moments"]
    assert m.shape == tuple(ref.shape) and m.dtype == torch.float32
    r = rel(m, ref)
    print(f"{key}: rel-L2(moments) = {r:.3e}")
    assert r < TOL


def test_encode_moments_256_both_groupnorm_modes(fx, dev):
    """2 x 256^2: the 128 -> 256 level's downsample GEMM (M = 8192, N = 256) is the first shape where the LINEAR
    GroupNorm-partials fusion engages; both modes of pdm_decoder_set_gn_fusion against the fixture."""
    lib = _lib.load()
    ae, x = _case(fx, "enc_full256")
    ae = ae.to(dev)
    ref = fx["enc_full256/moments"]
    fused = ae.encode_moments(x.to(dev)).cpu()
    try:
        assert lib.pdm_decoder_set_gn_fusion(0) == 0
        sep = ae.encode_moments(x.to(dev)).cpu()
    finally:
        lib.pdm_decoder_set_gn_fusion(1)
    rf, rs = rel(fused, ref), rel(sep, ref)
    print(f"enc_full256: rel-L2(moments) fused = {rf:.3e}, separate statistics = {rs:.3e}")
    assert rf < TOL
    assert rs < TOL


@pytest.mark.parametrize("key", ["enc64", "enc_full128"])
def test_sample_and_encode_vs_reference(fx, dev, key):
    ae, x = _case(fx, key)
    ae = ae.to(dev)
    noise = torch.from_numpy(fx[f"{key}/noise"]).to(dev)
    zref = fx[f"{key}/z"]
    z = ae.sample(torch.from_numpy(fx[f"{key}/moments"]).to(dev), noise=noise)
    assert z.shape == tuple(zref.shape)
    r = rel(z, zref)
    print(f"{key}: rel-L2(sample) = {r:.3e}")
    assert r < 1e-5
    r = rel(ae.encode(x.to(dev), noise=noise), zref)
    print(f"{key}: rel-L2(encode) = {r:.3e}")
    assert r < TOL


def test_sample_seeding_and_entry_points(fx, dev):
    ae, x = _case(fx, "enc64")
    ae = ae.to(dev)
    x = x.to(dev)
    m = ae.encode_moments(x)
    torch.manual_seed(123)
    a = ae.sample(m)
    torch.manual_seed(123)
    b = ae.sample(m)
    torch.manual_seed(123)
    noise = torch.randn_like(m[:, :4])
    assert torch.equal(a, b)
    assert torch.equal(a, ae.sample(m, noise=noise))
    g1, g2 = torch.Generator(device=dev).manual_seed(7), torch.Generator(device=dev).manual_seed(7)
    assert torch.equal(ae.sample(m, generator=g1), ae.sample(m, generator=g2))
    assert not torch.equal(ae.sample(m, generator=g1), a)
    # forward(inputs, fn) dispatch (libs/autoencoder.py:452-460)
    assert torch.equal(ae(x, "encode_moments"), m)
    torch.manual_seed(123)
    assert torch.equal(ae(x, "encode"), a)
    with pytest.raises(NotImplementedError):
        ae(x, "reconstruct")
    # the module-level helper is sample at scale 0.18215
    torch.manual_seed(123)
    assert torch.equal(AE.DiagonalGaussianDistribution(m), a)
    ae.scale_factor = 0.5
    torch.manual_seed(123)
    assert rel(ae.sample(m) * (0.18215 / 0.5), a) < 1e-6
    # logvar outside the clamp (libs/autoencoder.py:435)
    m2 = m.clone()
    m2[:, 4] = 50.0
    m2[:, 5] = -80.0
    mean, logvar = torch.chunk(m2, 2, dim=1)
    want = 0.5 * (mean + torch.exp(0.5 * torch.clamp(logvar, -30.0, 20.0)) * noise)
    assert rel(ae.sample(m2, noise=noise), want) < 1e-5


def test_encode_chunked_batch_matches_single(dev):
    """B = 5 at 48^2 in balanced chunks of <= 2 (2 + 2 + 1): every image equals the same image encoded alone."""
    ae = _ae(64, (1, 2), 1, 41, "random", encode_chunk=2).to(dev)
    x = _images(41, 5, 48).to(dev)
    m = ae.encode_moments(x)
    assert m.shape == (5, 8, 24, 24) and torch.isfinite(m).all()
    for i in range(5):
        assert rel(ae.encode_moments(x[i:i + 1]), m[i:i + 1]) < 1e-5


def test_encode_rejections(dev):
    with pytest.raises(ValueError):   # channel counts must be multiples of 64
        _ae(32, (1, 2), 1, 13, "random").to(dev).encode_moments(torch.zeros(1, 3, 48, 48, device=dev))
    full = _ae(128, (1, 2, 4, 4), 2, 14, "reference").to(dev)
    with pytest.raises(ValueError):   # latent 5: not a multiple of 8
        full.encode_moments(torch.zeros(1, 3, 40, 40, device=dev))
    with pytest.raises(ValueError):
        full.encode_moments(torch.zeros(1, 3, 64, 48, device=dev))
    with pytest.raises(RuntimeError):   # not on the GPU
        full.encode_moments(torch.zeros(1, 3, 64, 64))
    dec_only = _ae(64, (1, 2), 1, 15, "random", encoder=False).to(dev)
    with pytest.raises(RuntimeError, match="no encoder"):
        dec_only.encode_moments(torch.zeros(1, 3, 48, 48, device=dev))


def test_decoder_unchanged_by_encode_and_synthetic_encoder(dev):
    """One module: decode, encode, decode again -> bit-identical images; with synthetic weights the encoder is
    materialised on first use from encoder_spec and the module's seed."""
    dd = dict(W.DECODER_DDCONFIG, ch=64, ch_mult=[1, 2], num_res_blocks=1)
    ae = FrozenAutoencoderKL(dd, 4, seed=3, latent_size=24).to(dev)
    z = torch.randn(2, 4, 24, 24, generator=torch.Generator().manual_seed(2)).to(dev)
    before = ae.decode(z).clone()
    keys = list(ae.state_dict())
    m = ae.encode_moments(_images(3, 2, 48).to(dev))
    assert torch.equal(ae.decode(z), before)
    assert list(ae.state_dict()) == keys
    esd = W.encoder_state_dict(seed=3, ch=64, ch_mult=(1, 2), num_res_blocks=1)
    sd = W.make_state_dict(W.decoder_spec(ch=64, ch_mult=(1, 2), num_res_blocks=1), seed=3)
    same = FrozenAutoencoderKL(dd, 4, state_dict=dict(sd, **esd), latent_size=24).to(dev)
    assert torch.equal(same.encode_moments(_images(3, 2, 48).to(dev)), m)
    assert torch.equal(same.decode(z), before)
