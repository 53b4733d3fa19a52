"""Time the HIP KL-f8 encode (dev tool): python tools/encode_bench.py [B image_size [encode_chunk]]"""
import sys
import time

import torch

sys.path.insert(0, ".")
from panopticdiffusionmodels_amd import weights as W  # noqa: E402
from panopticdiffusionmodels_amd.libs.autoencoder import get_model  # noqa: E402


def encoder_flops(side, ch=128, ch_mult=(1, 2, 4, 4), num_res_blocks=2, in_channels=3, z_channels=4, double_z=True,
                  **_ignored):
    """Multiply-add FLOPs (2 per MAC) of Encoder.forward + quant_conv for one side x side image, from the config:
    every convolution (the GroupNorms, swishes and the softmax are not counted)."""
    fl, res, cin = 0, side, ch
    conv = lambda r, ci, co, k: 2 * r * r * ci * co * k * k  # noqa: E731
    fl += conv(res, in_channels, ch, 3)
    for lvl, m in enumerate(ch_mult):
        cout = ch * m
        for _ in range(num_res_blocks):
            fl += conv(res, cin, cout, 3) + conv(res, cout, cout, 3) + (conv(res, cin, cout, 1) if cin != cout else 0)
            cin = cout
        if lvl != len(ch_mult) - 1:
            res //= 2
            fl += conv(res, cin, cin, 3)
    fl += 4 * conv(res, cin, cin, 3)                      # mid.block_1, mid.block_2
    fl += 4 * conv(res, cin, cin, 1)                      # q, k, v, proj_out
    fl += 2 * 2 * (res * res) ** 2 * cin                  # q k^T and p v
    zc = 2 * z_channels if double_z else z_channels
    fl += conv(res, cin, zc, 3) + conv(res, zc, zc, 1)    # conv_out, quant_conv
    return fl


if __name__ == "__main__":
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    side = int(sys.argv[2]) if len(sys.argv) > 2 else 256
    chunk = int(sys.argv[3]) if len(sys.argv) > 3 else 8
    dev = torch.device("cuda")
    ae = get_model(None, seed=1, encode_chunk=chunk).to(dev)
    x = torch.rand(B, 3, side, side, device=dev) * 2 - 1
    for _ in range(2):
        ae.encode_moments(x)
    torch.cuda.synchronize()
    n = 5
    t0 = time.perf_counter()
    for _ in range(n):
        m = ae.encode_moments(x)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / n
    gf = encoder_flops(side, **W.ENCODER_DDCONFIG) / 1e9
    print(f"encode B={B} {side}x{side} (chunks of <= {chunk}): {dt*1e3:.1f} ms, {dt/B*1e3:.2f} ms/img, {B/dt:.1f} img/s, "
          f"{gf:.1f} GFLOP/img, {B*gf/dt/1e3:.1f} TFLOP/s, finite={bool(torch.isfinite(m).all())}")
