// KL-f8 encoder kernels (Encoder.forward, libs/autoencoder.py:275-300, quant_conv 419, sample 433-439) on gfx950: the
// layers the encoder does not share with the decoder.  The orchestration (pdm_encoder_* in decoder.hip) runs them
// around the decoder's resblock / attnblock / GroupNorm / GEMM layers.  A translation unit of its own, so the device
// code of every other source stays what it was.
#include <hip/hip_runtime.h>

#include "pdm_common.h"
#include "pdm_kernels.h"

namespace pdm {
namespace {

// Encoder conv_in (3 -> C, 3x3, pad 1): fp32 NCHW image -> fp32 NHWC residual stream.  K = 27 padded to 32: one
// v_mfma_f32_16x16x32_bf16 per 16 channels x 16 pixels, k = ci * 9 + ky * 3 + kx (the reference weight layout, so
// the fp32 [C][3][3][3] weight is registered unpacked and rounded to bf16 here).  The WEIGHTS are the first MFMA
// operand, so D[channel 4 * (lane / 16) + i][pixel lane % 16]: a lane holds 4 consecutive channels of one pixel
// and stores them as one 16-byte piece of the NHWC row.  A block owns one output row of one image (and up to 256
// output channels, blockIdx.z): the 3 channels x 3 rows x (W + 2) input halo and the bf16 weights are staged in
// LDS once, and the 4 waves walk the row in 16-pixel segments.
__global__ __launch_bounds__(256) void enc_conv_in_kernel(const float* img, const float* w, const float* bias,
                                                          float* out, int H, int W, int C) {
  __shared__ float rows[9 * 514];                                   // [ci * 3 + r][W + 2], W <= 512
  __shared__ __attribute__((aligned(16))) bf16 wl[256 * 32];       // [channel][k], k >= 27 zero
  const int y = blockIdx.x, b = blockIdx.y, c0 = blockIdx.z * 256, nc = min(256, C - c0);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, WP = W + 2;
  for (int e = threadIdx.x; e < 9 * WP; e += 256) {
    const int cr = e / WP, xx = e - cr * WP - 1, ci = cr / 3, yy = y + cr % 3 - 1;
    rows[e] = (yy >= 0 && yy < H && xx >= 0 && xx < W) ? img[(((size_t)b * 3 + ci) * H + yy) * W + xx] : 0.f;
  }
  for (int e = threadIdx.x; e < nc * 32; e += 256) {
    const int k = e & 31;
    wl[e] = k < 27 ? (bf16)w[(size_t)(c0 + (e >> 5)) * 27 + k] : (bf16)0.f;
  }
  __syncthreads();
  const int kq = (lane >> 4) * 8, px = lane & 15;
  int off[8];   // halo offset of the lane's 8 k values (-1: the zero padding of K)
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int k = kq + j;
    off[j] = k < 27 ? (k / 3) * WP + k % 3 : -1;   // k / 3 = ci * 3 + ky, k % 3 = kx
  }
  for (int x0 = wave * 16; x0 < W; x0 += 64) {
    const int x = x0 + px;
    bf16x8 pf;
#pragma unroll
    for (int j = 0; j < 8; ++j) pf[j] = (off[j] >= 0 && x < W) ? (bf16)rows[off[j] + x] : (bf16)0.f;
    // every lane runs the MFMAs; a lane past the row's end (W % 16 != 0) only skips its stores
    float* op = out + (((size_t)b * H + y) * W + x) * C + c0 + 4 * (lane >> 4);
    for (int cb = 0; cb < nc; cb += 16) {
      const bf16x8 wf = *reinterpret_cast<const bf16x8*>(wl + (cb + px) * 32 + kq);
      const f32x4 acc = mfma16x16x32(wf, pf, f32x4{0.f, 0.f, 0.f, 0.f});
      const f32x4 bo = *reinterpret_cast<const f32x4*>(bias + c0 + cb + 4 * (lane >> 4));
      if (x < W) *reinterpret_cast<f32x4*>(op + cb) = acc + bo;
    }
  }
}

// Downsample (libs/autoencoder.py:65-69: zero pad right / bottom by one, 3x3 stride-2 conv, padding 0) as a
// gather + the dense GEMM: X fp32 NHWC [B, H, W, C] -> A bf16 [B * (H/2) * (W/2)][9 * C], column (ky * 3 + kx) * C
// + ci of output pixel (y, x) = X[2y + ky][2x + kx][ci], zero at row H / column W.  One thread per 8 channels.
__global__ __launch_bounds__(256) void down_gather_kernel(const float* x, bf16* A, int H, int W, int C,
                                                          long long total) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int nq = C >> 3, per = 9 * nq, Ho = H >> 1, Wo = W >> 1;
  const long long m = i / per;
  const int r = (int)(i - m * per), tap = r / nq, q = r - tap * nq;
  const int b = (int)(m / ((long long)Ho * Wo)), p = (int)(m - (long long)b * Ho * Wo);
  const int yy = 2 * (p / Wo) + tap / 3, xx = 2 * (p % Wo) + tap % 3;
  bf16x8 o = bf16x8{};
  if (yy < H && xx < W) {
    const float* s = x + (((size_t)b * H + yy) * W + xx) * C + q * 8;
    const f32x4 t0 = *reinterpret_cast<const f32x4*>(s), t1 = *reinterpret_cast<const f32x4*>(s + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      o[j] = (bf16)t0[j];
      o[4 + j] = (bf16)t1[j];
    }
  }
  *reinterpret_cast<bf16x8*>(A + (size_t)i * 8) = o;
}

// Encoder tail: conv_out (C -> 8, 3x3, pad 1) on the GN + swish bf16 NHWC input, then quant_conv (8 -> 8, 1x1),
// written as the fp32 NCHW moments.  N = 8 is too narrow for the tile GEMMs (as the decoder's conv_out): a block
// owns 16 consecutive pixels, out[pixel][o] is the GEMM of the 9 * C im2col row with the [8][ky][kx][C] weight
// (the MFMA's columns o >= 8 are zero), the 9 * C / 32 k-steps are dealt round-robin to the 4 waves (the layer
// runs at the latent resolution: few pixels, long K), and the partial tiles are summed through LDS, where 128
// threads then apply the 1x1 quant_conv in fp32.
__global__ __launch_bounds__(256) void enc_tail_kernel(const bf16* g, int B, int H, int W, int C, const bf16* w,
                                                       const float* cbias, const float* qw, const float* qb,
                                                       float* moments) {
  __shared__ float part[4][16][9];   // [wave][pixel][o] (row padded to 9 floats)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int o = lane & 15, kq = (lane >> 4) * 8;
  const long long npix = (long long)B * H * W, m0 = (long long)blockIdx.x * 16;
  const long long m = m0 + (lane & 15);
  const bool live = m < npix;
  const int b = live ? (int)(m / ((long long)H * W)) : 0;
  const int r = live ? (int)(m - (long long)b * H * W) : 0, y = r / W, x = r - (r / W) * W;
  const int cs = C / 32, KS = 9 * cs;
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int ks = wave; ks < KS; ks += 4) {
    const int tap = ks / cs, c = (ks - tap * cs) * 32 + kq;
    const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
    bf16x8 a = bf16x8{}, wf = bf16x8{};
    if (live && yy >= 0 && yy < H && xx >= 0 && xx < W)
      a = *reinterpret_cast<const bf16x8*>(g + (((size_t)b * H + yy) * W + xx) * C + c);
    if (o < 8) wf = *reinterpret_cast<const bf16x8*>(w + (size_t)o * 9 * C + (size_t)tap * C + c);
    acc = mfma16x16x32(a, wf, acc);
  }
  // D[pixel 4 * (lane / 16) + i][o = lane % 16]
  if (o < 8)
#pragma unroll
    for (int i = 0; i < 4; ++i) part[wave][4 * (lane >> 4) + i][o] = acc[i];
  __syncthreads();
  if (threadIdx.x < 128) {
    const int p = threadIdx.x & 15, q = threadIdx.x >> 4;
    const long long mm = m0 + p;
    if (mm < npix) {
      float v = qb[q];
#pragma unroll
      for (int k = 0; k < 8; ++k)
        v = fmaf(qw[q * 8 + k], ((part[0][p][k] + part[1][p][k]) + (part[2][p][k] + part[3][p][k])) + cbias[k], v);
      const int bb = (int)(mm / ((long long)H * W));
      const int rr = (int)(mm - (long long)bb * H * W);
      moments[((size_t)bb * 8 + q) * H * W + rr] = v;
    }
  }
}

// FrozenAutoencoderKL.sample (libs/autoencoder.py:433-439): moments fp32 [B, 2C, hw] (mean = channels 0 .. C-1,
// logvar = C .. 2C-1), noise / z fp32 [B, C, hw]
__global__ __launch_bounds__(256) void moments_sample_kernel(const float* moments, const float* noise, float* z,
                                                             int C, int hw, float scale, long long total) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long long per = (long long)C * hw, b = i / per, r = i - b * per;
  const float mean = moments[b * 2 * per + r];
  const float logvar = fminf(fmaxf(moments[b * 2 * per + per + r], -30.0f), 20.0f);
  z[i] = scale * (mean + expf(0.5f * logvar) * noise[i]);
}

}  // namespace

hipError_t enc_conv_in_launch(const float* img, const float* w, const float* bias, float* out, int B, int H, int W,
                              int C, hipStream_t s) {
  if (W > 512 || C % 16) return hipErrorInvalidValue;   // the LDS halo rows hold W + 2 <= 514 pixels
  hipLaunchKernelGGL(enc_conv_in_kernel, dim3(H, B, (C + 255) / 256), dim3(256), 0, s, img, w, bias, out, H, W, C);
  return hipGetLastError();
}

hipError_t down_gather_launch(const float* x, bf16* A, int B, int H, int W, int C, hipStream_t s) {
  if (H % 2 || W % 2 || C % 8) return hipErrorInvalidValue;
  const long long total = (long long)B * (H / 2) * (W / 2) * 9 * (C / 8);
  hipLaunchKernelGGL(down_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, x, A, H, W, C, total);
  return hipGetLastError();
}

hipError_t enc_tail_launch(const bf16* g, int B, int H, int W, int C, const bf16* w, const float* cbias, const float* qw,
                           const float* qb, float* moments, hipStream_t s) {
  if (C % 32) return hipErrorInvalidValue;
  const long long npix = (long long)B * H * W;
  hipLaunchKernelGGL(enc_tail_kernel, dim3((unsigned)((npix + 15) / 16)), dim3(256), 0, s, g, B, H, W, C, w, cbias, qw,
                     qb, moments);
  return hipGetLastError();
}

hipError_t moments_sample_launch(const float* moments, const float* noise, float* z, int B, int C, int hw, float scale,
                                 hipStream_t s) {
  const long long total = (long long)B * C * hw;
  hipLaunchKernelGGL(moments_sample_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, moments, noise, z,
                     C, hw, scale, total);
  return hipGetLastError();
}

}  // namespace pdm
