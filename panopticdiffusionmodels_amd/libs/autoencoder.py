"""KL-f8 autoencoder — API of libs/autoencoder.py (`get_model(...)`: `decode(z)` 446-450, `encode_moments(x)` 428-431,
`sample(moments)` 433-439, `encode(x)` 441-444, `forward(inputs, fn)` 452-460, `DiagonalGaussianDistribution` 462-469).

`FrozenAutoencoderKL` keeps the reference's state_dict keys (`post_quant_conv.*`, `decoder.*`, `encoder.*`,
`quant_conv.*`), so `get_model(path)` loads the reference's assets/stable-diffusion/autoencoder_kl*.pth with
`torch.load(..., weights_only=True)`.  The decoder keys are required; the encoder keys are optional as a set (a
checkpoint with some but not all of them is an error; with none, `encode*` raises).  With synthetic weights
(`pretrained_path=None, state_dict=None`) the encoder weights are materialised from `weights.encoder_spec` and
the module's seed on the first encode, so decode-only callers construct exactly what they always did.

`decode` runs the hand-written HIP decoder of libpdm (csrc/decoder.hip, `pdm_decoder_*` in include/pdm.h):
NHWC activations, fp32 residual stream, every 3x3 conv an implicit GEMM on the bf16 MFMA GEMM kernels with
GroupNorm+swish fused into the producer of its bf16 input.  On first use the fp32 parameters are repacked
once (3x3 convs -> bf16 [Cout][ky][kx][Cin]; q/k/v -> one [3C, C] matrix; conv_out padded to 4 rows).
Large batches are decoded in chunks of at most `chunk` latents (the reference decodes in chunks of 50,
decode_large_batch in eval_ldm_discrete.py:62-68) so the workspace stays bounded.  The chunks are balanced (50 ->
25 + 25, not 32 + 18) and alternate over `lanes` streams -- the caller's and the process's shared lane streams
(_lib.lane_streams, the sampler's) -- with a workspace each, so two chunks decode at once and one's small
low-resolution launches fill the CUs the other leaves idle (B = 50: 47.3 -> 45.1 ms at 256^2, 183.0 -> 179.8 ms at
512^2; B = 32, split 16 + 16: 29.1 -> 28.3 ms, 116.4 -> 113.6 ms; bit-identical; tools/decode_lanes.py).

`encode_moments` runs the HIP encoder (`pdm_encoder_*`): the decoder's layers in the Encoder.forward order, a
bf16-MFMA conv_in, each stride-2 downsample as a gather into a bf16 [pixels][9 C] matrix plus the dense GEMM, and
conv_out + quant_conv in one kernel; weights repacked as for the decoder.  It encodes in balanced chunks of at most
`encode_chunk` images on the caller's stream.  `sample` is one elementwise kernel (`pdm_moments_sample`); its noise is
`torch.randn_like(mean)` unless `noise=` or `generator=` is given, so a seeded run consumes torch's RNG as the
reference does.
"""
import ctypes

import torch
import torch.nn as nn

from .. import _lib
from .. import weights as W

DDCONFIG = dict(W.DECODER_DDCONFIG)


class _DecoderHandle:
    """pdm_decoder handle + packed device copies of the weights it points at."""

    def __init__(self, module, device):
        lib = _lib.load()
        cfg = _lib.PdmDecoderCfg()
        cfg.ch = module.ch
        for i, m in enumerate(module.ch_mult):
            cfg.ch_mult[i] = m
        cfg.num_levels = len(module.ch_mult)
        cfg.num_res_blocks = module.num_res_blocks
        cfg.z_channels = module.z_channels
        cfg.out_ch = module.out_ch
        cfg.latent_size = module.latent_size
        cfg.scale_factor = module.scale_factor
        h = ctypes.c_void_p()
        _lib.check(lib.pdm_decoder_create(ctypes.byref(cfg), ctypes.byref(h)), "pdm_decoder_create")
        self.lib, self.h, self.device = lib, h, device
        self.packed = {}
        self.ws = {}         # lane -> workspace tensor
        self.ws_batch = {}
        buf = ctypes.create_string_buffer(256)
        for i in range(lib.pdm_decoder_param_count(h)):
            dt, numel = ctypes.c_int(), ctypes.c_longlong()
            _lib.check(lib.pdm_decoder_param_info(h, i, buf, 256, ctypes.byref(dt), ctypes.byref(numel)))
            name = buf.value.decode()
            t = self._pack(module, name, dt.value).to(device).contiguous()
            if t.numel() != numel.value:
                raise RuntimeError(f"decoder weight {name}: packed {t.numel()} elements, expected {numel.value}")
            self.packed[name] = t
            _lib.check(lib.pdm_decoder_set_param(h, name.encode(), _lib.ptr(t), dt.value, t.numel()),
                       "pdm_decoder_set_param")

    @staticmethod
    def _pack(m, name, dtype):
        if name.endswith("mid.attn_1.qkv.weight"):
            p = name[: -len("qkv.weight")]
            w = torch.cat([m._p(p + f"{n}.weight") for n in "qkv"]).reshape(-1, m._p(p + "q.weight").shape[1])
            return w.to(torch.bfloat16)
        if name.endswith("mid.attn_1.qkv.bias"):
            p = name[: -len("qkv.bias")]
            return torch.cat([m._p(p + f"{n}.bias") for n in "qkv"]).float()
        src = m._p(name).detach().float()
        if name == "decoder.conv_out.weight":   # [out_ch, C, 3, 3] -> [4][ky][kx][C], zero rows
            w = torch.zeros(4, *src.shape[1:], dtype=src.dtype, device=src.device)
            w[: src.shape[0]] = src
            return w.permute(0, 2, 3, 1).reshape(4, -1).to(torch.bfloat16)
        if name == "decoder.conv_out.bias":
            b = torch.zeros(4, dtype=src.dtype, device=src.device)
            b[: src.shape[0]] = src
            return b
        if dtype == _lib.PDM_BF16:
            if src.dim() == 4 and src.shape[-1] == 3:   # 3x3 conv -> [Cout][ky][kx][Cin]
                return src.permute(0, 2, 3, 1).reshape(src.shape[0], -1).to(torch.bfloat16)
            return src.reshape(src.shape[0], -1).to(torch.bfloat16)   # 1x1 conv
        return src.reshape(-1)

    def workspace(self, batch, lane=0):
        if self.ws.get(lane) is None or self.ws_batch[lane] < batch:
            nbytes = ctypes.c_size_t()
            _lib.check(self.lib.pdm_decoder_workspace_size(self.h, batch, ctypes.byref(nbytes)),
                       "pdm_decoder_workspace_size")
            self.ws[lane] = None
            self.ws[lane] = torch.empty(nbytes.value, dtype=torch.uint8, device=self.device)
            self.ws_batch[lane] = batch
        return self.ws[lane]

    def decode_into(self, z, img, n, lane, stream):
        ws = self.workspace(n, lane)
        _lib.check(self.lib.pdm_decoder_decode(self.h, _lib.ptr(z), _lib.ptr(img), n, _lib.ptr(ws), ws.numel(),
                                               stream), "pdm_decoder_decode")

    def __del__(self):
        try:
            self.lib.pdm_decoder_destroy(self.h)
        except Exception:
            pass


class _EncoderHandle:
    """pdm_encoder handle + packed device copies of the weights it points at (one per image size)."""

    def __init__(self, module, device, latent_size):
        lib = _lib.load()
        cfg = _lib.PdmEncoderCfg()
        cfg.ch = module.ch
        for i, m in enumerate(module.ch_mult[:4]):
            cfg.ch_mult[i] = m
        cfg.num_levels = len(module.ch_mult)
        cfg.num_res_blocks = module.num_res_blocks
        cfg.in_channels = module.in_channels
        cfg.z_channels = module.z_channels
        cfg.double_z = 1 if module.double_z else 0
        cfg.latent_size = latent_size
        h = ctypes.c_void_p()
        _lib.check(lib.pdm_encoder_create(ctypes.byref(cfg), ctypes.byref(h)), "pdm_encoder_create")
        self.lib, self.h, self.device, self.latent_size = lib, h, device, latent_size
        self.packed = {}
        self.ws = {}         # lane -> workspace tensor
        self.ws_batch = {}
        buf = ctypes.create_string_buffer(256)
        for i in range(lib.pdm_encoder_param_count(h)):
            dt, numel = ctypes.c_int(), ctypes.c_longlong()
            _lib.check(lib.pdm_encoder_param_info(h, i, buf, 256, ctypes.byref(dt), ctypes.byref(numel)))
            name = buf.value.decode()
            t = self._pack(module, name, dt.value).to(device).contiguous()
            if t.numel() != numel.value:
                raise RuntimeError(f"encoder weight {name}: packed {t.numel()} elements, expected {numel.value}")
            self.packed[name] = t
            _lib.check(lib.pdm_encoder_set_param(h, name.encode(), _lib.ptr(t), dt.value, t.numel()),
                       "pdm_encoder_set_param")

    @staticmethod
    def _pack(m, name, dtype):
        """The decoder's repacks: q/k/v -> one [3C, C] matrix, 3x3 convs (the stride-2 downsample and the 8-row
        conv_out included) -> bf16 [Cout][ky][kx][Cin], 1x1 convs -> bf16 [Cout][Cin]; conv_in, quant_conv, norms
        and biases stay fp32 in the reference layout."""
        return _DecoderHandle._pack(m, name, dtype)

    def workspace(self, batch, lane=0):
        if self.ws.get(lane) is None or self.ws_batch[lane] < batch:
            nbytes = ctypes.c_size_t()
            _lib.check(self.lib.pdm_encoder_workspace_size(self.h, batch, ctypes.byref(nbytes)),
                       "pdm_encoder_workspace_size")
            self.ws[lane] = None
            self.ws[lane] = torch.empty(nbytes.value, dtype=torch.uint8, device=self.device)
            self.ws_batch[lane] = batch
        return self.ws[lane]

    def encode_into(self, x, moments, n, lane, stream):
        ws = self.workspace(n, lane)
        _lib.check(self.lib.pdm_encoder_encode_moments(self.h, _lib.ptr(x), _lib.ptr(moments), n, _lib.ptr(ws),
                                                       ws.numel(), stream), "pdm_encoder_encode_moments")

    def __del__(self):
        try:
            self.lib.pdm_encoder_destroy(self.h)
        except Exception:
            pass


def _sample(moments, scale_factor, noise=None, generator=None):
    """z = scale * (mean + exp(0.5 * clamp(logvar, -30, 20)) * noise) on the HIP kernel (pdm_moments_sample)."""
    _lib.require_gpu(moments)
    if moments.dim() != 4 or moments.shape[1] % 2:
        raise ValueError(f"sample: expected moments [B, 2C, h, w], got {tuple(moments.shape)}")
    mean = moments[:, : moments.shape[1] // 2]
    if noise is None:
        if generator is None:
            noise = torch.randn_like(mean)   # libs/autoencoder.py:437
        else:
            noise = torch.randn(mean.shape, generator=generator, device=mean.device, dtype=mean.dtype)
    elif noise.shape != mean.shape or noise.device != moments.device:
        raise ValueError(f"sample: noise must be {tuple(mean.shape)} on {moments.device}")
    B, C, h, w = mean.shape
    m = moments.float().contiguous()
    n = noise.float().contiguous()
    z = torch.empty(B, C, h, w, dtype=torch.float32, device=m.device)
    if z.numel():
        _lib.check(_lib.load().pdm_moments_sample(_lib.ptr(m), _lib.ptr(n), _lib.ptr(z), B, C, h * w,
                                                  float(scale_factor), _lib.stream_ptr(m.device)), "pdm_moments_sample")
    return z.to(moments.dtype)


def DiagonalGaussianDistribution(moments):
    """libs/autoencoder.py:462-469 (scale_factor fixed at 0.18215)."""
    return _sample(moments, 0.18215)


class FrozenAutoencoderKL(nn.Module):
    def __init__(self, ddconfig=None, embed_dim=4, pretrained_path=None, scale_factor=0.18215, seed=0,
                 dtype=torch.bfloat16, state_dict=None, latent_size=32, chunk=32, lanes=2, encode_chunk=8):
        super().__init__()
        dd = dict(DDCONFIG if ddconfig is None else ddconfig)
        self.ch = int(dd["ch"])
        self.ch_mult = tuple(dd["ch_mult"])
        self.num_res_blocks = int(dd["num_res_blocks"])
        self.z_channels = int(dd["z_channels"])
        self.out_ch = int(dd["out_ch"])
        self.scale_factor = float(scale_factor)
        self.embed_dim = embed_dim
        self.compute_dtype = dtype
        self.latent_size = int(latent_size)
        self.chunk = int(chunk)
        self.lanes = max(1, int(lanes))
        self.encode_chunk = max(1, int(encode_chunk))
        self.in_channels = int(dd.get("in_channels", 3))
        self.double_z = bool(dd.get("double_z", True))
        self.seed = seed
        spec = W.decoder_spec(ch=self.ch, out_ch=self.out_ch, ch_mult=self.ch_mult,
                              num_res_blocks=self.num_res_blocks, z_channels=self.z_channels, embed_dim=embed_dim)
        if state_dict is not None or pretrained_path is not None:
            full = state_dict if state_dict is not None else torch.load(pretrained_path, map_location="cpu",
                                                                        weights_only=True)
            sd = {k: v for k, v in full.items() if k.startswith("decoder.") or k.startswith("post_quant_conv.")}
            missing = [k for k, _, _ in spec if k not in sd]
            if missing:
                raise RuntimeError(f"autoencoder checkpoint is missing {len(missing)} decoder keys, e.g. {missing[:3]}")
            # the encoder half is optional as a set: all of its keys, or none (then encode* raises)
            esd = {k: v for k, v in full.items() if k.startswith("encoder.") or k.startswith("quant_conv.")}
            if esd:
                emissing = [k for k in self._encoder_names() if k not in esd]
                if emissing:
                    raise RuntimeError(f"autoencoder checkpoint has encoder keys but is missing {len(emissing)} of "
                                       f"them, e.g. {emissing[:3]}")
            self._encoder = "loaded" if esd else "absent"
        else:
            sd = W.make_state_dict(spec, seed=seed, init="reference")
            esd = {}
            self._encoder = "synthetic"   # materialised on the first encode (_encoder_weights)
        self._names = [k for k, _, _ in spec]
        for k in self._names:
            self.register_buffer(k.replace(".", "__"), sd[k].float().clone())
        if esd:
            for k in self._encoder_names():
                self.register_buffer(k.replace(".", "__"), esd[k].float().clone())
        self.requires_grad_(False)
        self.eval()
        self._native = None
        self._enc_native = None

    def _encoder_names(self):
        return [k for k, _, _ in W.encoder_spec(ch=self.ch, ch_mult=self.ch_mult, num_res_blocks=self.num_res_blocks,
                                                z_channels=self.z_channels, embed_dim=self.embed_dim,
                                                in_channels=self.in_channels, double_z=self.double_z)]

    def _p(self, name):
        return getattr(self, name.replace(".", "__"))

    def _apply(self, fn, *a, **kw):
        self._native = None
        self._enc_native = None
        return super()._apply(fn, *a, **kw)

    def _load_from_state_dict(self, *a, **kw):
        self._native = None
        self._enc_native = None
        return super()._load_from_state_dict(*a, **kw)

    def native(self, device):
        if self._native is None or self._native.device != device:
            self._native = _DecoderHandle(self, device)
        return self._native

    @torch.no_grad()
    def decode(self, z):
        """libs/autoencoder.py:446-450 (z / scale_factor -> post_quant_conv -> Decoder.forward 376-409)."""
        _lib.require_gpu(z)
        B, C, h, w = z.shape
        if C != self.z_channels or h != self.latent_size or w != self.latent_size:
            if h == w and C == self.z_channels:   # another latent size: a handle per size
                self.latent_size = h
                self._native = None
            else:
                raise ValueError(f"decode: expected z [B, {self.z_channels}, s, s], got {tuple(z.shape)}")
        nat = self.native(z.device)
        z = z.float().contiguous()
        up = 2 ** (len(self.ch_mult) - 1)
        img = torch.empty(B, self.out_ch, h * up, w * up, dtype=torch.float32, device=z.device)
        # at least one chunk per lane once each gets >= 8 latents (B = 32: 16 + 16 concurrently, 29.1 -> 28.3 ms at 256^2)
        nch = max(-(-B // self.chunk), min(self.lanes, B // 8))
        sizes = [B // nch + (1 if i < B % nch else 0) for i in range(nch)]   # balanced chunks of <= chunk
        starts = [sum(sizes[:i]) for i in range(nch)]
        lanes = min(self.lanes, nch)
        if lanes == 1:
            stream = _lib.stream_ptr(z.device)
            for s0, n in zip(starts, sizes):
                nat.decode_into(z[s0:s0 + n], img[s0:s0 + n], n, 0, stream)
            return img
        # chunk i on lane i % lanes: lane 0 the caller's stream, lanes 1.. the process's shared side streams (the
        # sampler's lane streams, _lib.lane_streams: no new hardware queue); the side lanes start behind everything
        # queued on the caller's stream and the caller's stream waits for them at the end
        main = torch.cuda.current_stream(z.device)
        streams = [main] + _lib.lane_streams(z.device, lanes - 1)
        for st in streams[1:]:
            st.wait_stream(main)
        for i, (s0, n) in enumerate(zip(starts, sizes)):
            lane = i % lanes
            nat.decode_into(z[s0:s0 + n], img[s0:s0 + n], n, lane, ctypes.c_void_p(streams[lane].cuda_stream))
        for st in streams[1:]:
            main.wait_stream(st)
        return img

    def _encoder_weights(self, device):
        if self._encoder == "absent":
            raise RuntimeError("encode: the weights this autoencoder was built from hold no encoder "
                               "(no encoder.* / quant_conv.* keys)")
        if self._encoder == "synthetic":
            # seeded on the CPU generator (the same values on every device), then placed on the input's device
            spec = W.encoder_spec(ch=self.ch, ch_mult=self.ch_mult, num_res_blocks=self.num_res_blocks,
                                  z_channels=self.z_channels, embed_dim=self.embed_dim,
                                  in_channels=self.in_channels, double_z=self.double_z)
            esd = W.make_state_dict(spec, seed=self.seed, init="reference")
            for k, v in esd.items():
                self.register_buffer(k.replace(".", "__"), v.float().to(device), persistent=False)
            self._encoder = "loaded"

    def native_encoder(self, device, latent_size):
        n = self._enc_native
        if n is None or n.device != device or n.latent_size != latent_size:
            self._enc_native = None
            self._encoder_weights(device)
            self._enc_native = _EncoderHandle(self, device, latent_size)
        return self._enc_native

    @torch.no_grad()
    def encode_moments(self, x):
        """libs/autoencoder.py:428-431 (Encoder.forward 275-300 -> quant_conv): x [B, 3, S, S] -> [B, 8, S/f, S/f]."""
        _lib.require_gpu(x)
        f = 2 ** (len(self.ch_mult) - 1)
        if x.dim() != 4 or x.shape[1] != self.in_channels or x.shape[2] != x.shape[3] or x.shape[2] % f:
            raise ValueError(f"encode_moments: expected x [B, {self.in_channels}, S, S] with S a multiple of {f}, "
                             f"got {tuple(x.shape)}")
        B, S = x.shape[0], x.shape[2]
        if self._encoder == "absent":
            self._encoder_weights(x.device)
        nat = self.native_encoder(x.device, S // f)
        xf = x.float().contiguous()
        moments = torch.empty(B, 2 * self.z_channels, S // f, S // f, dtype=torch.float32, device=x.device)
        if B == 0:
            return moments
        nch = -(-B // self.encode_chunk)
        sizes = [B // nch + (1 if i < B % nch else 0) for i in range(nch)]   # balanced chunks of <= encode_chunk
        stream = _lib.stream_ptr(x.device)
        s0 = 0
        for n in sizes:
            nat.encode_into(xf[s0:s0 + n], moments[s0:s0 + n], n, 0, stream)
            s0 += n
        return moments

    def sample(self, moments, noise=None, generator=None):
        """libs/autoencoder.py:433-439."""
        return _sample(moments, self.scale_factor, noise=noise, generator=generator)

    def encode(self, x, noise=None, generator=None):
        """libs/autoencoder.py:441-444."""
        return self.sample(self.encode_moments(x), noise=noise, generator=generator)

    def forward(self, inputs, fn):
        if fn == "encode_moments":
            return self.encode_moments(inputs)
        if fn == "encode":
            return self.encode(inputs)
        if fn == "decode":
            return self.decode(inputs)
        raise NotImplementedError(fn)


def get_model(pretrained_path=None, scale_factor=0.18215, **kw):
    """libs/autoencoder.py:471-484 (pretrained_path=None -> synthetic seeded weights)."""
    return FrozenAutoencoderKL(DDCONFIG, 4, pretrained_path, scale_factor, **kw)
