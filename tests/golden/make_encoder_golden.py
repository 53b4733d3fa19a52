"""Generate tests/golden/encoder_golden.npz: the REFERENCE Encoder + quant_conv (libs/autoencoder.py:209-300, 419,
428-431) in fp32 on the CPU, on this repo's seeded weights (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_encoder_golden.py <reference checkout>

Arrays only.  Per case <key> of CASES (tests/test_gpu_encoder.py runs the same table):
  <key>/moments       encode_moments of the case's images
  <key>/img_sum       float64 sum of every image (the images themselves are drawn on both sides from a seeded CPU
                      generator, uniform(-1, 1): a generator mismatch fails loudly instead of as a parity error)
  <key>/sd_checksum   weights checksum (make_golden._sd_checksum)
  <key>/noise, <key>/z   a fixed noise and the reference's sample(moments) with it (libs/autoencoder.py:433-439,
                      scale_factor 0.18215)
and `state_dict_keys`: the reference FrozenAutoencoderKL's encoder.* / quant_conv.* keys in state_dict order (full
ddconfig).  Nothing here is imported by the product or run on the GPU box; the .npz is data.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import W, _import_reference, _np, _sd_checksum  # noqa: E402

# key, ch, ch_mult, num_res_blocks, weight seed, init, batch, image side
CASES = [
    ("enc64", 64, (1, 2), 1, 31, "random", 3, 48),
    ("enc_full128", 128, (1, 2, 4, 4), 2, 32, "reference", 1, 128),
    ("enc_full256", 128, (1, 2, 4, 4), 2, 33, "random", 2, 256),
    ("enc_full512", 128, (1, 2, 4, 4), 2, 34, "reference", 1, 512),
]
SCALE = 0.18215


def images(seed, batch, side):
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.rand(batch, 3, side, side, generator=g) * 2.0 - 1.0


def ddconfig(ch, mult, nrb):
    return dict(double_z=True, z_channels=4, resolution=256, in_channels=3, out_ch=3, ch=ch, ch_mult=list(mult),
                num_res_blocks=nrb, attn_resolutions=[], dropout=0.0)


def main():
    if len(sys.argv) != 2:
        sys.exit("usage: make_encoder_golden.py <reference checkout>")
    ref = sys.argv[1]
    ae = _import_reference(ref)[2]
    torch.set_num_threads(16)
    out = {}
    for key, ch, mult, nrb, seed, init, batch, side in CASES:
        sd = W.encoder_state_dict(seed=seed, init=init, ch=ch, ch_mult=mult, num_res_blocks=nrb)
        enc = ae.Encoder(**ddconfig(ch, mult, nrb))
        enc.load_state_dict({k[len("encoder."):]: v for k, v in sd.items() if k.startswith("encoder.")})
        enc.eval()
        qc = torch.nn.Conv2d(8, 8, 1)
        qc.load_state_dict({"weight": sd["quant_conv.weight"], "bias": sd["quant_conv.bias"]})
        x = images(seed, batch, side)
        with torch.no_grad():
            moments = qc(enc(x))   # FrozenAutoencoderKL.encode_moments, libs/autoencoder.py:428-431
        g = torch.Generator().manual_seed(2000 + seed)
        mean, logvar = torch.chunk(moments, 2, dim=1)
        noise = torch.randn(mean.shape, generator=g)
        z = SCALE * (mean + torch.exp(0.5 * torch.clamp(logvar, -30.0, 20.0)) * noise)   # sample, 433-439
        out[f"{key}/moments"] = _np(moments)
        out[f"{key}/img_sum"] = np.array([float(x[i].double().sum()) for i in range(batch)], dtype=np.float64)
        out[f"{key}/sd_checksum"] = _sd_checksum(sd)
        out[f"{key}/noise"] = _np(noise)
        out[f"{key}/z"] = _np(z)
        print(key, tuple(moments.shape), float(moments.abs().mean()), flush=True)

    # the reference's own key list: build the whole FrozenAutoencoderKL module tree without its checkpoint load
    full = ddconfig(128, (1, 2, 4, 4), 2)
    m = torch.nn.Module()
    m.encoder = ae.Encoder(**full)
    m.decoder = ae.Decoder(**full)
    m.quant_conv = torch.nn.Conv2d(8, 8, 1)
    m.post_quant_conv = torch.nn.Conv2d(4, 4, 1)
    keys = [k for k in m.state_dict().keys() if k.startswith("encoder.") or k.startswith("quant_conv.")]
    out["state_dict_keys"] = np.array(keys)
    path = os.path.join(HERE, "encoder_golden.npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in out.items()})
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
