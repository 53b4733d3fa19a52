// KL-f8 decoder (libs/autoencoder.py:303-409 + FrozenAutoencoderKL.decode 446-450) on gfx950.
//
// Activations are NHWC; the residual stream is fp32, every conv input is a bf16 NHWC tensor produced by a
// fused GroupNorm(32)+swish apply (or a plain cast).  Every 3x3 conv is an implicit GEMM on the U-ViT GEMM
// kernels (conv mode: per-row tap addressing, padded taps read a zero page, the nearest-x2 upsample folded
// into the source address), with bias and the residual add fused into the epilogue (EPI_F32 accumulate
// into the residual stream).  The mid attention block (single head over h*w tokens, C = 512) runs as a
// packed qkv GEMM, batched Q K^T / P V GEMMs and a row softmax.
//
// The KL-f8 encoder (libs/autoencoder.py:209-300 + quant_conv, FrozenAutoencoderKL.encode_moments 428-431) is the
// second half of this file: the same layers in Encoder.forward order plus the kernels of encoder.hip (conv_in, the
// stride-2 downsample's gather in front of the dense GEMM, the conv_out + quant_conv tail, and the elementwise
// FrozenAutoencoderKL.sample).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "../../include/pdm.h"
#include "pdm_common.h"
#include "pdm_kernels.h"

using pdm::bf16;

namespace pdm {
namespace {

// ---------------------------------------------------------------------------------------------------
// GroupNorm statistics: grid (nchunk, B); each block reduces `pix` pixels x C channels in fp64 (sum, sumsq)
// per group, partials -> [B, nchunk, 32, 2]; gn_final combines them into (mean, rstd) per (b, g).  pix is chosen
// per level so that a block streams ~256 KiB (gn_pix below): 64-pixel chunks left every block latency-bound.
constexpr int GN_PIX = 64;   // smallest chunk (sizes the partials buffer)
inline int gn_pix(int C) { return C >= 1024 ? GN_PIX : 65536 / C; }

template <typename T>
__global__ __launch_bounds__(256) void gn_partial_kernel(const T* x, int P, int C, int nchunk, int pix, double* part) {
  // thread -> one channel quad q of pixel lane `plane` (C <= 1024): per-channel fp32 sums over its <= pix/planes
  // pixels in registers (compile-time indexed: a runtime group index sent the accumulators to scratch), then
  // one fp64 pass per group over the [plane][channel] partials in LDS
  __shared__ float2 red[1024];
  const int b = blockIdx.y, chunk = blockIdx.x;
  const int nq = C >> 2, q = threadIdx.x % nq, plane = threadIdx.x / nq, planes = 256 / nq;
  const int p0 = chunk * pix, p1 = min(P, p0 + pix);
  if (plane < planes) {
    const T* xb = x + (size_t)b * P * C + q * 4;
    float su[4] = {0.f, 0.f, 0.f, 0.f}, sq[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int pi = p0 + plane; pi < p1; pi += planes) {
      float v[4];
      if constexpr (sizeof(T) == 4) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(xb + (size_t)pi * C);
        v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
      } else {
        const bf16x4 t = *reinterpret_cast<const bf16x4*>(xb + (size_t)pi * C);
        v[0] = (float)t[0]; v[1] = (float)t[1]; v[2] = (float)t[2]; v[3] = (float)t[3];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        su[j] += v[j];
        sq[j] = fmaf(v[j], v[j], sq[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) red[plane * C + q * 4 + j] = make_float2(su[j], sq[j]);
  }
  __syncthreads();
  if (threadIdx.x < 32) {
    const int g = threadIdx.x, cpg = C / 32;
    double s = 0.0, qq = 0.0;
    for (int pl = 0; pl < planes; ++pl)
      for (int c = g * cpg; c < (g + 1) * cpg; ++c) {
        const float2 r = red[pl * C + c];
        s += r.x;
        qq += r.y;
      }
    double* o = part + (((size_t)b * nchunk + chunk) * 32 + g) * 2;
    o[0] = s;
    o[1] = qq;
  }
}

// one wave per (b, g): lanes stride over the chunks, then a wave reduction (a serial per-thread loop over the
// chunks was a chain of dependent global loads, ~135 us per call)
__global__ __launch_bounds__(256) void gn_final_kernel(const double* part, int nchunk, double count, float eps,
                                                       float* stats, int B) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;   // (b, g)
  if (i >= B * 32) return;
  const int b = i / 32, g = i % 32;
  double s = 0.0, q = 0.0;
  for (int c = lane; c < nchunk; c += 64) {
    const double* o = part + (((size_t)b * nchunk + c) * 32 + g) * 2;
    s += o[0];
    q += o[1];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_xor(s, o, 64);
    q += __shfl_xor(q, o, 64);
  }
  if (lane) return;
  const double mean = s / count;
  double var = q / count - mean * mean;
  var = var < 0.0 ? 0.0 : var;
  stats[i * 2] = (float)mean;
  stats[i * 2 + 1] = (float)(1.0 / sqrt(var + (double)eps));
}

// y = [swish]((x - mean) * rstd * gamma + beta), NHWC, bf16 out.  Grid (gx, B): a block stays in one image and
// every thread keeps one channel octet q (C <= 2048, C % 8 == 0) for all its pixels, so the per-channel affine
// a = rstd * gamma, b = beta - mean * a is folded once into registers and the pixel loop is two 16-byte loads
// (fp32; one for bf16), one FMA + swish per element and one 16-byte store, 32-bit indexing only.  (The first
// version decoded (image, pixel, channel) from a flat 64-bit index per element and reloaded stats, gamma and
// beta per element: ~40 % of HBM bandwidth.)  swish = u / (1 + 2^(-u log2 e)) with the hardware exp2 and
// reciprocal (u -> -inf gives -0, no NaN).
template <typename T>
__global__ __launch_bounds__(256) void gn_apply_kernel(const T* x, const float* stats, const float* gamma,
                                                       const float* beta, bf16* y, int P, int C, int swish) {
  const int no = C >> 3, planes = 256 / no, q = threadIdx.x % no, plane = threadIdx.x / no;
  if (plane >= planes) return;
  const int b = blockIdx.y, c = q * 8, cpg = C / 32;
  float a[8], o[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int g = (c + j) / cpg;   // cpg may be 2 or 6: an octet can straddle groups
    const float mean = stats[(b * 32 + g) * 2], rstd = stats[(b * 32 + g) * 2 + 1];
    a[j] = rstd * gamma[c + j];
    o[j] = fmaf(-mean, a[j], beta[c + j]);
  }
  const T* xb = x + (size_t)b * P * C + c;
  bf16* yb = y + (size_t)b * P * C + c;
  const int step = gridDim.x * planes;
#pragma unroll 4
  for (int pi = blockIdx.x * planes + plane; pi < P; pi += step) {
    float v[8];
    if constexpr (sizeof(T) == 4) {
      const f32x4 t0 = *reinterpret_cast<const f32x4*>(xb + (size_t)pi * C);
      const f32x4 t1 = *reinterpret_cast<const f32x4*>(xb + (size_t)pi * C + 4);
      v[0] = t0[0]; v[1] = t0[1]; v[2] = t0[2]; v[3] = t0[3];
      v[4] = t1[0]; v[5] = t1[1]; v[6] = t1[2]; v[7] = t1[3];
    } else {
      const bf16x8 t = *reinterpret_cast<const bf16x8*>(xb + (size_t)pi * C);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (float)t[j];
    }
    bf16x8 r;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float u = fmaf(v[j], a[j], o[j]);
      if (swish) u *= __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(u * -1.4426950408889634f));
      r[j] = (bf16)u;
    }
    *reinterpret_cast<bf16x8*>(yb + (size_t)pi * C) = r;
  }
}

// z [B, 4, h, w] fp32 -> z / scale -> post_quant_conv (1x1, 4->4) -> conv_in (3x3, 4->Cout) -> NHWC fp32
__global__ __launch_bounds__(256) void conv_in_kernel(const float* z, float inv_scale, const float* pq_w,
                                                      const float* pq_b, const float* w, const float* bias,
                                                      float* out, int h, int wd, int Cout) {
  const int b = blockIdx.y, y = blockIdx.x;
  __shared__ float rows[3][4][66];   // 3 input rows x 4 channels x (w + 2 halo), post_quant applied
  for (int e = threadIdx.x; e < 3 * 4 * (wd + 2); e += 256) {
    const int r = e / (4 * (wd + 2)), rem = e % (4 * (wd + 2)), c = rem / (wd + 2), xx = rem % (wd + 2) - 1;
    const int yy = y + r - 1;
    float v = 0.f;
    if (yy >= 0 && yy < h && xx >= 0 && xx < wd) {
      v = pq_b[c];
      for (int ci = 0; ci < 4; ++ci) v += pq_w[c * 4 + ci] * z[(((size_t)b * 4 + ci) * h + yy) * wd + xx] * inv_scale;
    }
    rows[r][c][xx + 1] = v;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < wd * Cout; e += 256) {
    const int x = e / Cout, co = e % Cout;
    float acc = bias[co];
    const float* wp = w + (size_t)co * 36;
    for (int ci = 0; ci < 4; ++ci)
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) acc = fmaf(wp[ci * 9 + ky * 3 + kx], rows[ky][ci][x + kx], acc);
    out[(((size_t)b * h + y) * wd + x) * Cout + co] = acc;
  }
}

// row softmax of fp32 scores * scale -> bf16 probabilities (rows of n <= 4096), one block per row; the row is
// read once into registers (16 values per thread; the three-pass form re-read it for the max, the sum and
// the output: 1.38 ms for 32 x 4096 rows of 4096)
__global__ __launch_bounds__(256) void softmax_rows_kernel(const float* s, bf16* p, int n, float scale) {
  const float* row = s + (size_t)blockIdx.x * n;
  bf16* out = p + (size_t)blockIdx.x * n;
  __shared__ float red[8];
  float v[16];
  float m = -3.0e38f;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int i = threadIdx.x + j * 256;
    v[j] = i < n ? row[i] * scale : -3.0e38f;
    m = fmaxf(m, v[j]);
  }
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    v[j] = __expf(v[j] - m);   // 0 past n
    sum += v[j];
  }
  sum = wave_sum(sum);
  if ((threadIdx.x & 63) == 0) red[4 + (threadIdx.x >> 6)] = sum;
  __syncthreads();
  const float inv = 1.0f / ((red[4] + red[5]) + (red[6] + red[7]));
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int i = threadIdx.x + j * 256;
    if (i < n) out[i] = (bf16)(v[j] * inv);
  }
}

// [B][n][ld] column block -> [B][C][n] transpose (bf16), 32x32 tiles through LDS
__global__ __launch_bounds__(256) void transpose_kernel(const bf16* src, int ld, int col0, bf16* dst, int n, int C) {
  __shared__ bf16 t[32][33];
  const int b = blockIdx.z;
  const int r0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const bf16* s = src + (size_t)b * n * ld + col0;
  bf16* d = dst + (size_t)b * C * n;
  for (int i = threadIdx.x; i < 1024; i += 256) {
    const int r = i / 32, c = i % 32;
    t[r][c] = s[(size_t)(r0 + r) * ld + c0 + c];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 1024; i += 256) {
    const int c = i / 32, r = i % 32;
    d[(size_t)(c0 + c) * n + r0 + r] = t[r][c];
  }
}

// conv_out (libs/autoencoder.py:408-409): 3x3 conv, Cin -> out_ch <= 4, on the GN+swish bf16 NHWC input, written
// straight to the NCHW fp32 image.  N = 3 is far too narrow for an MFMA tile (a 128-wide tile wastes 97 % of
// its work), so one thread computes one pixel's outputs on the VALU: 9 taps x Cin/8 16-byte loads (neighbour
// rows come from L1 / L2); the weights are staged once per block into LDS as fp32 [tap][ci][4 outputs], so each
// input channel costs one broadcast ds_read_b128 + 4 FMAs (per-lane weight loads from global cost 4x the input
// bandwidth).
__global__ __launch_bounds__(256) void conv_out_kernel(const bf16* g, int B, int H, int W, int C, const bf16* w,
                                                       const float* bias, float* img, int out_ch) {
  extern __shared__ __attribute__((aligned(16))) f32x4 wl[];   // [9 * C]
  for (int i = threadIdx.x; i < 9 * C; i += 256)
    wl[i] = f32x4{(float)w[i], (float)w[9 * C + i], (float)w[18 * C + i], (float)w[27 * C + i]};
  __syncthreads();
  const long long pix = (long long)blockIdx.x * 256 + threadIdx.x;
  if (pix >= (long long)B * H * W) return;
  const int b = (int)(pix / ((long long)H * W));
  const int r = (int)(pix - (long long)b * H * W), y = r / W, x = r - (r / W) * W;
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int tap = 0; tap < 9; ++tap) {
    const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
    if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
    const bf16* src = g + (((size_t)b * H + yy) * W + xx) * C;
    const f32x4* wt = wl + tap * C;
    for (int c0 = 0; c0 < C; c0 += 8) {
      const bf16x8 v = *reinterpret_cast<const bf16x8*>(src + c0);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc += (float)v[j] * wt[c0 + j];
    }
  }
  for (int o = 0; o < out_ch; ++o) img[((size_t)b * out_ch + o) * H * W + r] = acc[o] + bias[o];
}

// The same conv for C in {64, 128} (every shipped decoder) on the matrix cores: out[pixel][o] is a GEMM of the
// 9 * C im2col row with a 9C x 16 weight block (o >= out_ch zero), one v_mfma_f32_16x16x32_bf16 per 32-channel
// slice of a tap.  A block owns two output rows of one image and walks them in 64-pixel segments (4 waves x 16
// pixels x 2 rows); per segment the 4 x 66 halo of input pixels is staged in LDS once by LDS-DMA (every input
// pixel was re-read by 9 taps from L2 in the VALU version: 4.7 ms for 32 images at 512^2; register-staged loads
// with one load in flight per thread: 1.9 ms), each pixel's 16-byte channel chunks XOR-swizzled by the pixel
// index so the 16 lanes of an A-fragment read (16 consecutive pixels, one chunk) hit distinct banks.  The DMA
// writes lane-linearly, so the swizzle is applied to the SOURCE chunk; halo pixels outside the image read as
// zeros through the buffer descriptor's range check.  Two blocks per CU (68 KiB of LDS each) overlap one's
// staging with the other's MFMAs.  A lane keeps its B fragments (w[o = lane % 16][k-slice]) for the whole K in
// registers.
template <int C>
__global__ __launch_bounds__(256) void conv_out_mfma_kernel(const bf16* g, int H, int W, const bf16* w,
                                                            const float* bias, float* img, int out_ch) {
  constexpr int NQ = C / 8;                  // 16-byte chunks per pixel
  constexpr int SW = (NQ < 16 ? NQ : 16) - 1;
  constexpr int SEG = 64, PX = SEG + 2;      // output pixels per segment, staged pixels per row
  constexpr int SLOTS = 4 * PX * NQ;         // 16-byte LDS slots per segment (4 input rows)
  constexpr int KS = 9 * C / 32;             // MFMA k-steps (a k-step never straddles a tap: C % 32 == 0)
  static_assert(SLOTS % 64 == 0, "every LDS-DMA wave-instruction lands 64 slots inside the tile");
  __shared__ __attribute__((aligned(16))) bf16 tile[SLOTS * 8];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int y0 = blockIdx.x * 2, b = blockIdx.y;
  const int o = lane & 15, kq = (lane >> 4) * 8;
  bf16x8 wf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    wf[ks] = bf16x8{};
    if (o < out_ch) wf[ks] = *reinterpret_cast<const bf16x8*>(w + (size_t)o * 9 * C + ks * 32 + kq);
  }
  const float bo = o < out_ch ? bias[o] : 0.f;
  const long long img_bytes = (long long)H * W * C * 2;
  const __amdgpu_buffer_rsrc_t rg = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<bf16*>(g + (size_t)b * H * W * C), 0, (int)(img_bytes < 0x7fffffffLL ? img_bytes : 0x7fffffffLL), 0x00020000);
  for (int x0 = 0; x0 < W; x0 += SEG) {
    // slot e = (r * PX + px) * NQ + s holds logical chunk s ^ (px & SW) of input pixel (y0 - 1 + r, x0 - 1 + px)
    for (int e0 = wave * 64; e0 < SLOTS; e0 += 256) {
      const int e = e0 + lane;
      const int r = e / (PX * NQ), rem = e - r * (PX * NQ), px = rem / NQ, sl = rem - px * NQ;
      const int yy = y0 + r - 1, xx = x0 + px - 1;
      const unsigned off = (e < SLOTS && yy >= 0 && yy < H && xx >= 0 && xx < W)
                               ? (unsigned)((yy * W + xx) * C + ((sl ^ (px & SW)) << 3)) * 2u : 0x80000000u;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rg, (PDM_LDS void*)(tile + e0 * 8), 16, (int)off, 0, 0, 0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    f32x4 acc0 = f32x4{0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int dy = tap / 3, dx = tap - (tap / 3) * 3;
      const int px = wave * 16 + (lane & 15) + dx;
#pragma unroll
      for (int c0 = 0; c0 < C; c0 += 32) {
        const int q = (c0 + kq) >> 3;
        const int sw = (q ^ (px & SW)) * 8;
        const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(tile + (dy * PX + px) * NQ * 8 + sw);
        const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(tile + ((dy + 1) * PX + px) * NQ * 8 + sw);
        acc0 = mfma16x16x32(a0, wf[tap * (C / 32) + c0 / 32], acc0);
        acc1 = mfma16x16x32(a1, wf[tap * (C / 32) + c0 / 32], acc1);
      }
    }
    // D[pixel 4 * (lane / 16) + i][o = lane % 16]: 4 consecutive pixels of output channel o
    if (o < out_ch) {
      float* op = img + (((size_t)b * out_ch + o) * H + y0) * W + x0 + wave * 16 + 4 * (lane >> 4);
      *reinterpret_cast<f32x4*>(op) = acc0 + bo;
      *reinterpret_cast<f32x4*>(op + W) = acc1 + bo;
    }
    __syncthreads();   // every wave is done reading the tile before the next segment restages it
  }
}

// ---------------------------------------------------------------------------------------------------
// Launches: grid, shared-memory size and kernel choice of every kernel above, each in ONE place -- the decoder /
// encoder orchestration below and the pdm_vae_* entry points (parity tests on caller-owned tensors) both go through
// them.  Each returns hipErrorInvalidValue for a shape its kernel cannot take.
inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// GroupNorm(32): statistics pass (skipped with part_ready: `part` then holds partials in 256-pixel chunks, as the GEMM
// epilogue leaves them), (mean, rstd) -> stats [B, 32, 2], apply -> y.  part: B * gn_chunks(P, C, part_ready) * 64
// doubles.
inline int gn_chunks(int P, int C, bool part_ready) {
  const int pix = part_ready ? 256 : gn_pix(C);
  return (P + pix - 1) / pix;
}
inline bool gn_shape_ok(int B, int P, int C) {
  // gn_partial_kernel: one thread per channel quad, >= 1 pixel plane per block, red[] holds planes * C <= 1024 sums;
  // gn_apply_kernel: one thread per channel octet; blockIdx.y = image
  return B > 0 && B <= 65535 && P > 0 && C > 0 && C % 32 == 0 && C <= 1024;
}
template <typename T>
hipError_t gn_launch(const T* x, int B, int P, int C, const float* gamma, const float* beta, float eps, bool swish,
                     double* part, bool part_ready, float* stats, bf16* y, hipStream_t s) {
  if (!gn_shape_ok(B, P, C) || (part_ready && P % 256)) return hipErrorInvalidValue;
  const int pix = part_ready ? 256 : gn_pix(C);
  const int nchunk = gn_chunks(P, C, part_ready);
  if (!part_ready)
    hipLaunchKernelGGL(gn_partial_kernel<T>, dim3(nchunk, B), dim3(256), 0, s, x, P, C, nchunk, pix, part);
  hipLaunchKernelGGL(gn_final_kernel, dim3((B * 32 + 3) / 4), dim3(256), 0, s, part, nchunk, (double)P * (C / 32), eps,
                     stats, B);
  const int planes = 256 / (C / 8);
  // >= ~8192 blocks (up to 32 waves per CU): the pixel loop keeps 4 pixels' loads in flight per thread, and at
  // ~2048 blocks the fp32 apply streamed at ~2.5 TB/s (512^2 decode, profiles/r03r_dec512_kernel_stats.csv)
  const int gx = std::max(1, std::min((P + planes - 1) / planes, 8192 / B + 1));
  hipLaunchKernelGGL(gn_apply_kernel<T>, dim3(gx, B), dim3(256), 0, s, x, stats, gamma, beta, y, P, C, swish ? 1 : 0);
  return hipGetLastError();
}

// decoder z -> post_quant_conv -> conv_in: the LDS rows hold w + 2 <= 66 pixels
hipError_t dec_conv_in_launch(const float* z, float scale_factor, const float* pq_w, const float* pq_b, const float* w,
                              const float* bias, float* out, int B, int h, int wd, int Cout, hipStream_t s) {
  if (B <= 0 || B > 65535 || h <= 0 || wd <= 0 || wd > 64 || Cout <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(conv_in_kernel, dim3(h, B), dim3(256), 0, s, z, 1.0f / scale_factor, pq_w, pq_b, w, bias, out, h,
                     wd, Cout);
  return hipGetLastError();
}

// row softmax: a row lives in 16 registers x 256 threads
hipError_t softmax_rows_launch(const float* sc, bf16* p, long long rows, int n, float scale, hipStream_t s) {
  if (rows <= 0 || rows > 0x7fffffffLL || n <= 0 || n > 4096) return hipErrorInvalidValue;
  hipLaunchKernelGGL(softmax_rows_kernel, dim3((unsigned)rows), dim3(256), 0, s, sc, p, n, scale);
  return hipGetLastError();
}

// [B][n][ld] columns col0 .. col0 + C -> [B][C][n]: whole 32 x 32 tiles only
hipError_t transpose_launch(const bf16* src, int ld, int col0, bf16* dst, int B, int n, int C, hipStream_t s) {
  if (B <= 0 || B > 65535 || n <= 0 || n % 32 || C <= 0 || C % 32 || C / 32 > 65535 || col0 < 0 || col0 + C > ld)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(transpose_kernel, dim3(n / 32, C / 32, B), dim3(256), 0, s, src, ld, col0, dst, n, C);
  return hipGetLastError();
}

// decoder conv_out: the MFMA kernel for C in {64, 128} on whole 64-pixel segments and row pairs (every shipped
// decoder), else -- or with force_valu (parity tests) -- the VALU kernel, whose fp32 weights take 9 * C * 16 bytes of
// dynamic LDS
inline bool conv_out_mfma(int B, int H, int W, int C, bool force_valu) {
  return !force_valu && (C == 128 || C == 64) && W % 64 == 0 && H % 2 == 0 && B <= 65535;
}
hipError_t conv_out_launch(const bf16* g, int B, int H, int W, int C, const bf16* w, const float* bias, float* img,
                           int out_ch, bool force_valu, hipStream_t s) {
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8 || out_ch < 1 || out_ch > 4) return hipErrorInvalidValue;
  const bool mfma = conv_out_mfma(B, H, W, C, force_valu);
  if (mfma && C == 128)
    hipLaunchKernelGGL(conv_out_mfma_kernel<128>, dim3(H / 2, B), dim3(256), 0, s, g, H, W, w, bias, img, out_ch);
  else if (mfma)
    hipLaunchKernelGGL(conv_out_mfma_kernel<64>, dim3(H / 2, B), dim3(256), 0, s, g, H, W, w, bias, img, out_ch);
  else {
    const long long npix = (long long)B * H * W;
    hipLaunchKernelGGL(conv_out_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 9 * C * 16, s, g, B, H, W, C, w,
                       bias, img, out_ch);
  }
  return hipGetLastError();
}

}  // namespace
}  // namespace pdm

// =====================================================================================================
namespace {

int dfail(int code, const std::string& m) { return pdm::set_error(code, m); }
#define D_HIP(call)                                                                                   \
  do {                                                                                                \
    hipError_t e_ = (call);                                                                           \
    if (e_ != hipSuccess) return dfail(PDM_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
  } while (0)
#define D_CHECK(m)                              \
  do {                                          \
    const char* m_ = (m);                       \
    if (m_) return dfail(PDM_ERR_ARG, m_);      \
  } while (0)
#define D_TRY(x)        \
  do {                  \
    int r_ = (x);       \
    if (r_) return r_;  \
  } while (0)

struct DParam {
  int dtype;
  long long numel;
  const void* ptr = nullptr;
};

}  // namespace

struct pdm_decoder {
  pdm_decoder_cfg cfg;
  int nlev, top_ch, h0;
  std::vector<std::string> order;
  std::map<std::string, DParam> params;
  void add(const std::string& n, int dt, long long ne) {
    order.push_back(n);
    params[n] = DParam{dt, ne, nullptr};
  }
  const float* f(const std::string& n) const { return (const float*)params.at(n).ptr; }
  const bf16* w(const std::string& n) const { return (const bf16*)params.at(n).ptr; }
  void add_res(const std::string& p, int cin, int cout) {
    add(p + ".norm1.weight", PDM_F32, cin);
    add(p + ".norm1.bias", PDM_F32, cin);
    add(p + ".conv1.weight", PDM_BF16, 9LL * cin * cout);
    add(p + ".conv1.bias", PDM_F32, cout);
    add(p + ".norm2.weight", PDM_F32, cout);
    add(p + ".norm2.bias", PDM_F32, cout);
    add(p + ".conv2.weight", PDM_BF16, 9LL * cout * cout);
    add(p + ".conv2.bias", PDM_F32, cout);
    if (cin != cout) {
      add(p + ".nin_shortcut.weight", PDM_BF16, 1LL * cin * cout);
      add(p + ".nin_shortcut.bias", PDM_F32, cout);
    }
  }
};

namespace {

struct DWork {
  float* X;       // residual stream fp32 NHWC (max pixels x channels)
  float* X2;      // second residual buffer (nin shortcut / upsample output)
  bf16* G;        // bf16 conv input
  bf16* H;        // bf16 conv1 output
  bf16* XB;       // bf16 copy of X for the next block's nin_shortcut, written by the producing conv's epilogue
  bf16* QKV;      // attention: [B*hw, 3C]
  float* S;       // attention scores [B, hw, hw]
  bf16* P;        // probabilities [B, hw, hw]
  bf16* VT;       // V^T [B, C, hw]
  bf16* O;        // attention output [B*hw, C]
  double* part;   // GN partials
  float* stats;   // GN (mean, rstd) [B, 32, 2]
  bf16* zero;     // 256 zero bytes
  bf16* A;        // encoder only: the downsample's gathered GEMM operand [B * (H/2) * (W/2), 9 C]
  size_t bytes;
};

size_t aup(size_t x) { return (x + 255) / 256 * 256; }
using pdm::GN_PIX;

DWork dlayout(const pdm_decoder* d, int B, char* base) {
  DWork w{};
  size_t off = 0;
  auto take = [&](size_t n) {
    char* p = base ? base + off : nullptr;
    off = aup(off + n);
    return p;
  };
  // largest activation: after the last upsample, 2^(nlev-1) * h0 squared pixels x the preceding level's C
  size_t maxe = 0;
  int res = d->h0, cin = d->top_ch;
  for (int lvl = d->nlev - 1; lvl >= 0; --lvl) {
    const int cout = d->cfg.ch * d->cfg.ch_mult[lvl];
    size_t e = (size_t)res * res * (cin > cout ? cin : cout);
    if (e > maxe) maxe = e;
    cin = cout;
    if (lvl != 0) {
      res *= 2;
      e = (size_t)res * res * cin;
      if (e > maxe) maxe = e;
    }
  }
  const size_t hw = (size_t)d->h0 * d->h0;
  w.X = (float*)take((size_t)B * maxe * 4);
  w.X2 = (float*)take((size_t)B * maxe * 4);
  w.G = (bf16*)take((size_t)B * maxe * 2);
  w.H = (bf16*)take((size_t)B * maxe * 2);
  w.XB = (bf16*)take((size_t)B * maxe * 2);
  w.QKV = (bf16*)take((size_t)B * hw * 3 * d->top_ch * 2);
  w.S = (float*)take((size_t)B * hw * hw * 4);
  w.P = (bf16*)take((size_t)B * hw * hw * 2);
  w.VT = (bf16*)take((size_t)B * hw * d->top_ch * 2);
  w.O = (bf16*)take((size_t)B * hw * d->top_ch * 2);
  w.part = (double*)take((size_t)B * ((size_t)res * res / GN_PIX + 1) * 32 * 2 * sizeof(double));
  w.stats = (float*)take((size_t)B * 32 * 2 * 4);
  w.zero = (bf16*)take(256);
  w.bytes = off;
  return w;
}

struct DCtx {
  const pdm_decoder* d;
  hipStream_t s;
  const DWork* w;
  // set by the GEMM / conv that just wrote the next GroupNorm's input with GemmArgs::gn_part (its partials in w->part,
  // 256-pixel chunks), cleared by the GroupNorm that consumes them
  bool* gn_ready;
};

template <typename T>
int groupnorm(const DCtx& c, const T* x, int B, int P, int C, const std::string& norm, bf16* y, bool swish) {
  // statistics pass: skipped when the producing epilogue already left the partials (one read of x fewer)
  const bool pre = *c.gn_ready;
  *c.gn_ready = false;
  if (!pdm::gn_shape_ok(B, P, C)) return dfail(PDM_ERR_ARG, "decoder: GroupNorm needs C % 32 == 0 and C <= 1024");
  D_HIP(pdm::gn_launch<T>(x, B, P, C, c.d->f(norm + ".weight"), c.d->f(norm + ".bias"), 1e-6f, swish, c.w->part, pre,
                          c.w->stats, y, c.s));
  return PDM_OK;
}

// implicit-GEMM conv3x3 (in: bf16 NHWC [B, res>>up, res>>up, cin]) -> epilogue
bool g_gn_fusion = true;   // pdm_decoder_set_gn_fusion

// gn_P > 0: the output is the next GroupNorm's input (gn_P pixels per image): its epilogue also writes the GroupNorm
// partials where it can (pdm::gemm_gn_fusable; c.gn_ready tells the GroupNorm)
// (shared with pdm_gemm_bf16_gn / pdm_gemm_conv3x3_bf16_gn; *fused: whether the epilogue wrote `part`)
int gemm_gn(pdm::GemmArgs& a, int epi, double* part, int gn_P, hipStream_t s, bool* fused) {
  if (gn_P > 0 && g_gn_fusion) {
    a.gn_part = part; a.gn_P = gn_P; a.gn_cpg = a.N / 32;
    if (!pdm::gemm_gn_fusable(a, epi)) a.gn_part = nullptr;
  }
  D_CHECK(pdm::gemm_check(a, epi));
  D_HIP(pdm::gemm_launch(a, epi, s));
  *fused = a.gn_part != nullptr;
  return PDM_OK;
}

int launch_gn(const DCtx& c, pdm::GemmArgs& a, int epi, int gn_P) {
  return gemm_gn(a, epi, c.w->part, gn_P, c.s, c.gn_ready);
}

// the implicit-GEMM operands of a conv3x3 over a B x H x W output grid (H, W after the optional x2 upsample)
pdm::GemmArgs conv3_args(const bf16* in, int B, int H, int W, int cin, int up, const bf16* wt, const float* bias,
                         int cout, bf16* ob, float* of, int accumulate, const bf16* zero) {
  pdm::GemmArgs a{};
  a.A1 = in; a.lda1 = cin; a.K1 = 9 * cin;
  a.W = wt; a.bias = bias;
  a.M = B * H * W; a.N = cout; a.K = 9 * cin;
  a.out_bf16 = ob; a.ldo = cout; a.out_f32 = of; a.ldr = cout; a.accumulate = accumulate;
  a.conv = 1; a.convH = H; a.convW = W; a.convC = cin; a.conv_up = up; a.zero = zero;
  return a;
}

int conv3(const DCtx& c, const bf16* in, int B, int res, int cin, int cout, const std::string& name, int epi,
          bf16* ob, float* of, int accumulate, int up = 0, bool gn = false) {
  pdm::GemmArgs a = conv3_args(in, B, res, res, cin, up, c.d->w(name + ".weight"), c.d->f(name + ".bias"), cout, ob, of,
                               accumulate, c.w->zero);
  return launch_gn(c, a, epi, gn ? res * res : 0);
}

int linear(const DCtx& c, const bf16* A, int M, int K, const bf16* W, const float* bias, int N, int epi, bf16* ob,
           float* of, int accumulate, int gn_P = 0) {
  pdm::GemmArgs a{};
  a.A1 = A; a.lda1 = K; a.K1 = K; a.W = W; a.bias = bias; a.M = M; a.N = N; a.K = K;
  a.out_bf16 = ob; a.ldo = N; a.out_f32 = of; a.ldr = N; a.accumulate = accumulate;
  return launch_gn(c, a, epi, gn_P);
}

// ResnetBlock (libs/autoencoder.py:75-134): X (fp32 NHWC, cin) -> X (cout) in place (or via X2 for nin).
// xb: bf16(X) already made by the epilogue that produced X (else the nin_shortcut casts X itself); copy_out:
// where conv2's epilogue also stores bf16 of the block output (the next upsample conv's source), or null.
int resblock(const DCtx& c, float*& X, float*& X2, int B, int res, int cin, int cout, const std::string& p,
             const bf16* xb = nullptr, bf16* copy_out = nullptr) {
  const DWork& w = *c.w;
  const int P = res * res;
  D_TRY(groupnorm<float>(c, X, B, P, cin, p + ".norm1", w.G, true));
  D_TRY(conv3(c, w.G, B, res, cin, cout, p + ".conv1", pdm::EPI_BF16, w.H, nullptr, 0, 0, true));
  D_TRY(groupnorm<bf16>(c, w.H, B, P, cout, p + ".norm2", w.G, true));
  if (cin != cout) {
    // x = nin_shortcut(x): 1x1 conv = GEMM on a bf16 copy of x, into X2; then X2 += conv2(h)
    if (!xb) {
      D_HIP(pdm::cast_bf16_launch(X, w.H, (long long)B * P * cin, c.s));
      xb = w.H;
    }
    D_TRY(linear(c, xb, B * P, cin, c.d->w(p + ".nin_shortcut.weight"), c.d->f(p + ".nin_shortcut.bias"), cout,
                 pdm::EPI_F32, nullptr, X2, 0));
    D_TRY(conv3(c, w.G, B, res, cout, cout, p + ".conv2", pdm::EPI_F32, copy_out, X2, 1, 0, true));
    float* t = X;
    X = X2;
    X2 = t;
  } else {
    D_TRY(conv3(c, w.G, B, res, cout, cout, p + ".conv2", pdm::EPI_F32, copy_out, X, 1, 0, true));
  }
  return PDM_OK;
}

// AttnBlock (libs/autoencoder.py:143-195), single head over hw tokens, channels C
int attnblock(const DCtx& c, float* X, int B, int res, int C, const std::string& p) {
  const DWork& w = *c.w;
  const int hw = res * res;
  D_TRY(groupnorm<float>(c, X, B, hw, C, p + ".norm", w.G, false));
  D_TRY(linear(c, w.G, B * hw, C, c.d->w(p + ".qkv.weight"), c.d->f(p + ".qkv.bias"), 3 * C, pdm::EPI_BF16, w.QKV,
               nullptr, 0));
  {  // S[b] = Q[b] K[b]^T  (batched over b)
    pdm::GemmArgs a{};
    a.A1 = w.QKV; a.lda1 = 3 * C; a.K1 = C;
    a.W = w.QKV + C; a.ldw = 3 * C;
    a.M = hw; a.N = hw; a.K = C;
    a.out_f32 = w.S; a.ldr = hw;
    a.batch = B; a.sA = (long long)hw * 3 * C; a.sW = (long long)hw * 3 * C; a.sR = (long long)hw * hw;
    D_CHECK(pdm::gemm_check(a, pdm::EPI_F32));
    D_HIP(pdm::gemm_launch(a, pdm::EPI_F32, c.s));
  }
  D_HIP(pdm::softmax_rows_launch(w.S, w.P, (long long)B * hw, hw, 1.0f / sqrtf((float)C), c.s));
  D_HIP(pdm::transpose_launch(w.QKV, 3 * C, 2 * C, w.VT, B, hw, C, c.s));
  {  // O[b] = P[b] V[b]  with V^T as the [N][K] operand
    pdm::GemmArgs a{};
    a.A1 = w.P; a.lda1 = hw; a.K1 = hw;
    a.W = w.VT;
    a.M = hw; a.N = C; a.K = hw;
    a.out_bf16 = w.O; a.ldo = C;
    a.batch = B; a.sA = (long long)hw * hw; a.sW = (long long)C * hw; a.sO = (long long)hw * C;
    D_CHECK(pdm::gemm_check(a, pdm::EPI_BF16));
    D_HIP(pdm::gemm_launch(a, pdm::EPI_BF16, c.s));
  }
  // x + proj_out(o)
  D_TRY(linear(c, w.O, B * hw, C, c.d->w(p + ".proj_out.weight"), c.d->f(p + ".proj_out.bias"), C, pdm::EPI_F32,
               nullptr, X, 1, hw));
  return PDM_OK;
}

}  // namespace

extern "C" {

int pdm_decoder_create(const pdm_decoder_cfg* cfg, pdm_decoder** out) {
  if (!cfg || !out) return dfail(PDM_ERR_ARG, "pdm_decoder_create: null argument");
  const pdm_decoder_cfg& c = *cfg;
  if (c.num_levels < 1 || c.num_levels > 4) return dfail(PDM_ERR_ARG, "decoder: 1..4 levels supported");
  if (c.z_channels != 4) return dfail(PDM_ERR_ARG, "decoder: z_channels must be 4");
  if (c.out_ch > 4) return dfail(PDM_ERR_ARG, "decoder: out_ch must be <= 4");
  for (int i = 0; i < c.num_levels; ++i)
    if ((c.ch * c.ch_mult[i]) % 64) return dfail(PDM_ERR_ARG, "decoder: channel counts must be multiples of 64");
  if (c.latent_size % 8 || c.latent_size > 64) return dfail(PDM_ERR_ARG, "decoder: latent size must be a multiple of 8, <= 64");
  for (int i = 0; i < c.num_levels; ++i)
    if (c.ch * c.ch_mult[i] > 1024) return dfail(PDM_ERR_ARG, "decoder: channel counts must be <= 1024");
  pdm_decoder* d = new pdm_decoder();
  d->cfg = c;
  d->nlev = c.num_levels;
  d->top_ch = c.ch * c.ch_mult[c.num_levels - 1];
  d->h0 = c.latent_size;
  const int T = d->top_ch;
  d->add("post_quant_conv.weight", PDM_F32, 16);
  d->add("post_quant_conv.bias", PDM_F32, 4);
  d->add("decoder.conv_in.weight", PDM_F32, (long long)T * 36);
  d->add("decoder.conv_in.bias", PDM_F32, T);
  d->add_res("decoder.mid.block_1", T, T);
  d->add("decoder.mid.attn_1.norm.weight", PDM_F32, T);
  d->add("decoder.mid.attn_1.norm.bias", PDM_F32, T);
  d->add("decoder.mid.attn_1.qkv.weight", PDM_BF16, 3LL * T * T);
  d->add("decoder.mid.attn_1.qkv.bias", PDM_F32, 3LL * T);
  d->add("decoder.mid.attn_1.proj_out.weight", PDM_BF16, 1LL * T * T);
  d->add("decoder.mid.attn_1.proj_out.bias", PDM_F32, T);
  d->add_res("decoder.mid.block_2", T, T);
  int cin = T;
  for (int lvl = d->nlev - 1; lvl >= 0; --lvl) {
    const int cout = c.ch * c.ch_mult[lvl];
    for (int b = 0; b <= c.num_res_blocks; ++b) {
      d->add_res("decoder.up." + std::to_string(lvl) + ".block." + std::to_string(b), cin, cout);
      cin = cout;
    }
    if (lvl != 0) {
      d->add("decoder.up." + std::to_string(lvl) + ".upsample.conv.weight", PDM_BF16, 9LL * cin * cin);
      d->add("decoder.up." + std::to_string(lvl) + ".upsample.conv.bias", PDM_F32, cin);
    }
  }
  d->add("decoder.norm_out.weight", PDM_F32, cin);
  d->add("decoder.norm_out.bias", PDM_F32, cin);
  d->add("decoder.conv_out.weight", PDM_BF16, 4LL * 9 * cin);   // padded to 4 output rows
  d->add("decoder.conv_out.bias", PDM_F32, 4);
  *out = d;
  return PDM_OK;
}

int pdm_decoder_set_gn_fusion(int on) {
  g_gn_fusion = on != 0;
  return PDM_OK;
}

int pdm_decoder_destroy(pdm_decoder* d) {
  delete d;
  return PDM_OK;
}

int pdm_decoder_param_count(const pdm_decoder* d) { return d ? (int)d->order.size() : 0; }

int pdm_decoder_param_info(const pdm_decoder* d, int i, char* name, int len, int* dtype, long long* numel) {
  if (!d || i < 0 || i >= (int)d->order.size()) return dfail(PDM_ERR_ARG, "pdm_decoder_param_info: index out of range");
  snprintf(name, len, "%s", d->order[i].c_str());
  *dtype = d->params.at(d->order[i]).dtype;
  *numel = d->params.at(d->order[i]).numel;
  return PDM_OK;
}

int pdm_decoder_set_param(pdm_decoder* d, const char* name, const void* ptr, int dtype, long long numel) {
  if (!d || !name) return dfail(PDM_ERR_ARG, "pdm_decoder_set_param: null argument");
  auto it = d->params.find(name);
  if (it == d->params.end()) return dfail(PDM_ERR_ARG, std::string("pdm_decoder_set_param: unexpected key ") + name);
  if (it->second.dtype != dtype || it->second.numel != numel)
    return dfail(PDM_ERR_ARG, std::string("pdm_decoder_set_param: dtype/size mismatch for ") + name);
  if ((uintptr_t)ptr & 15) return dfail(PDM_ERR_ARG, std::string("pdm_decoder_set_param: unaligned ") + name);
  it->second.ptr = ptr;
  return PDM_OK;
}

int pdm_decoder_workspace_size(const pdm_decoder* d, int B, size_t* bytes) {
  if (!d || B <= 0 || !bytes) return dfail(PDM_ERR_ARG, "pdm_decoder_workspace_size: bad argument");
  *bytes = dlayout(d, B, nullptr).bytes;
  return PDM_OK;
}

int pdm_decoder_decode(pdm_decoder* d, const float* z, float* img, int B, void* workspace, size_t workspace_bytes,
                       void* stream) {
  if (!d || !z || !img || B <= 0) return dfail(PDM_ERR_ARG, "pdm_decoder_decode: bad argument");
  for (auto& n : d->order)
    if (!d->params[n].ptr) return dfail(PDM_ERR_STATE, "pdm_decoder: weight not registered: " + n);
  DWork w = dlayout(d, B, (char*)workspace);
  if (w.bytes > workspace_bytes) return dfail(PDM_ERR_ARG, "pdm_decoder_decode: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  bool gn_ready = false;
  DCtx c{d, s, &w, &gn_ready};
  D_HIP(hipMemsetAsync(w.zero, 0, 256, s));
  const int T = d->top_ch;
  int res = d->h0;
  float* X = w.X;
  float* X2 = w.X2;
  D_HIP(pdm::dec_conv_in_launch(z, d->cfg.scale_factor, d->f("post_quant_conv.weight"), d->f("post_quant_conv.bias"),
                                d->f("decoder.conv_in.weight"), d->f("decoder.conv_in.bias"), X, B, res, res, T, s));
  D_TRY(resblock(c, X, X2, B, res, T, T, "decoder.mid.block_1"));
  D_TRY(attnblock(c, X, B, res, T, "decoder.mid.attn_1"));
  D_TRY(resblock(c, X, X2, B, res, T, T, "decoder.mid.block_2"));
  int cin = T;
  const bf16* xb = nullptr;   // bf16(X) from the epilogue that produced X, when the next block's nin needs it
  for (int lvl = d->nlev - 1; lvl >= 0; --lvl) {
    const int cout = d->cfg.ch * d->cfg.ch_mult[lvl];
    for (int b = 0; b <= d->cfg.num_res_blocks; ++b) {
      // the level's last block also stores bf16 of its output into H: the upsample conv's source (H is free
      // once norm2 has consumed conv1's output)
      bf16* cp = (b == d->cfg.num_res_blocks && lvl != 0) ? w.H : nullptr;
      D_TRY(resblock(c, X, X2, B, res, cin, cout, "decoder.up." + std::to_string(lvl) + ".block." + std::to_string(b),
                     cin != cout ? xb : nullptr, cp));
      xb = nullptr;
      cin = cout;
    }
    if (lvl != 0) {  // nearest x2 upsample folded into the conv's source addressing (35-50)
      res *= 2;
      const int next = d->cfg.ch * d->cfg.ch_mult[lvl - 1];
      bf16* cp = next != cin ? w.XB : nullptr;   // the next level's first block changes width: its nin input
      D_TRY(conv3(c, w.H, B, res, cin, cin, "decoder.up." + std::to_string(lvl) + ".upsample.conv", pdm::EPI_F32,
                  cp, X2, 0, 1, true));
      xb = cp;
      float* t = X;
      X = X2;
      X2 = t;
    }
  }
  D_TRY(groupnorm<float>(c, X, B, res * res, cin, "decoder.norm_out", w.G, true));
  D_HIP(pdm::conv_out_launch(w.G, B, res, res, cin, d->w("decoder.conv_out.weight"), d->f("decoder.conv_out.bias"), img,
                             d->cfg.out_ch, false, s));
  return PDM_OK;
}


}  // extern "C"

// =====================================================================================================
// KL-f8 encoder: FrozenAutoencoderKL.encode_moments (libs/autoencoder.py:428-431) = Encoder.forward (275-300) ->
// quant_conv.  The layer set is the decoder's (resblock, attnblock, groupnorm, the implicit-GEMM conv3 and the dense
// linear above, with the same GroupNorm-partials protocol); new are conv_in, the downsample gather and the tail.
struct pdm_encoder {
  pdm_encoder_cfg cfg;
  int nlev, top_ch, side;
  pdm_decoder tab;   // the parameter table (names, dtypes, device pointers) in the form the shared layers read
};

namespace {

DWork elayout(const pdm_encoder* e, int B, char* base, size_t* a_bytes = nullptr) {
  DWork w{};
  size_t off = 0;
  auto take = [&](size_t n) {
    char* p = base ? base + off : nullptr;
    off = aup(off + n);
    return p;
  };
  // largest activation and largest gathered downsample operand over the levels
  size_t maxe = 0, maxa = 0;
  int res = e->side, cin = e->cfg.ch;
  for (int lvl = 0; lvl < e->nlev; ++lvl) {
    const int cout = e->cfg.ch * e->cfg.ch_mult[lvl];
    maxe = std::max(maxe, (size_t)res * res * std::max(cin, cout));
    cin = cout;
    if (lvl != e->nlev - 1) {
      maxa = std::max(maxa, (size_t)(res / 2) * (res / 2) * 9 * cin);
      res /= 2;
    }
  }
  const size_t hw = (size_t)res * res;
  const int T = e->top_ch;
  w.X = (float*)take((size_t)B * maxe * 4);
  w.X2 = (float*)take((size_t)B * maxe * 4);
  w.G = (bf16*)take((size_t)B * maxe * 2);
  w.H = (bf16*)take((size_t)B * maxe * 2);
  w.A = (bf16*)take((size_t)B * maxa * 2);
  if (a_bytes) *a_bytes = (size_t)B * maxa * 2;
  w.QKV = (bf16*)take((size_t)B * hw * 3 * T * 2);
  w.S = (float*)take((size_t)B * hw * hw * 4);
  w.P = (bf16*)take((size_t)B * hw * hw * 2);
  w.VT = (bf16*)take((size_t)B * hw * T * 2);
  w.O = (bf16*)take((size_t)B * hw * T * 2);
  w.part = (double*)take((size_t)B * ((size_t)e->side * e->side / GN_PIX + 1) * 32 * 2 * sizeof(double));
  w.stats = (float*)take((size_t)B * 32 * 2 * 4);
  w.zero = (bf16*)take(256);
  w.bytes = off;
  return w;
}

// Downsample.forward (libs/autoencoder.py:65-69): X (fp32 NHWC, res x res x C) -> X2 (res/2 x res/2 x C), swapped
int downsample(const DCtx& c, float*& X, float*& X2, int B, int res, int C, const std::string& p) {
  const int ro = res / 2;
  const long long M = (long long)B * ro * ro;
  D_HIP(pdm::down_gather_launch(X, c.w->A, B, res, res, C, c.s));
  D_TRY(linear(c, c.w->A, (int)M, 9 * C, c.d->w(p + ".weight"), c.d->f(p + ".bias"), C, pdm::EPI_F32, nullptr, X2, 0,
               ro * ro));
  float* t = X;
  X = X2;
  X2 = t;
  return PDM_OK;
}

}  // namespace

extern "C" {

int pdm_encoder_create(const pdm_encoder_cfg* cfg, pdm_encoder** out) {
  if (!cfg || !out) return dfail(PDM_ERR_ARG, "pdm_encoder_create: null argument");
  const pdm_encoder_cfg& c = *cfg;
  if (c.num_levels < 1 || c.num_levels > 4) return dfail(PDM_ERR_ARG, "encoder: 1..4 levels supported");
  if (c.in_channels != 3) return dfail(PDM_ERR_ARG, "encoder: in_channels must be 3");
  if (c.z_channels != 4 || !c.double_z) return dfail(PDM_ERR_ARG, "encoder: z_channels must be 4 with double_z");
  if (c.num_res_blocks < 1) return dfail(PDM_ERR_ARG, "encoder: num_res_blocks must be >= 1");
  if (c.ch <= 0 || c.ch % 64 || c.ch > 1024)
    return dfail(PDM_ERR_ARG, "encoder: channel counts must be multiples of 64, <= 1024");
  for (int i = 0; i < c.num_levels; ++i)
    if (c.ch_mult[i] <= 0 || (c.ch * c.ch_mult[i]) % 64 || c.ch * c.ch_mult[i] > 1024)
      return dfail(PDM_ERR_ARG, "encoder: channel counts must be multiples of 64, <= 1024");
  if (c.latent_size <= 0 || c.latent_size % 8 || (c.latent_size << (c.num_levels - 1)) > 512)
    return dfail(PDM_ERR_ARG, "encoder: latent size must be a multiple of 8 and the image side "
                              "latent * 2^(levels - 1) at most 512");
  // the mid AttnBlock's row softmax holds a row of latent^2 scores in registers (softmax_rows_launch): without this a
  // one- or two-level encoder above latent 64 would normalise over the first 4096 keys only
  if (c.latent_size > 64)
    return dfail(PDM_ERR_ARG, "encoder: latent size must be <= 64 (the attention softmax takes at most 4096 tokens)");
  pdm_encoder* e = new pdm_encoder();
  e->cfg = c;
  e->nlev = c.num_levels;
  e->top_ch = c.ch * c.ch_mult[c.num_levels - 1];
  e->side = c.latent_size << (c.num_levels - 1);
  pdm_decoder& d = e->tab;
  const int T = e->top_ch;
  d.add("encoder.conv_in.weight", PDM_F32, 27LL * c.ch);
  d.add("encoder.conv_in.bias", PDM_F32, c.ch);
  int cin = c.ch;
  for (int lvl = 0; lvl < e->nlev; ++lvl) {
    const int cout = c.ch * c.ch_mult[lvl];
    for (int b = 0; b < c.num_res_blocks; ++b) {
      d.add_res("encoder.down." + std::to_string(lvl) + ".block." + std::to_string(b), cin, cout);
      cin = cout;
    }
    if (lvl != e->nlev - 1) {
      d.add("encoder.down." + std::to_string(lvl) + ".downsample.conv.weight", PDM_BF16, 9LL * cin * cin);
      d.add("encoder.down." + std::to_string(lvl) + ".downsample.conv.bias", PDM_F32, cin);
    }
  }
  d.add_res("encoder.mid.block_1", T, T);
  d.add("encoder.mid.attn_1.norm.weight", PDM_F32, T);
  d.add("encoder.mid.attn_1.norm.bias", PDM_F32, T);
  d.add("encoder.mid.attn_1.qkv.weight", PDM_BF16, 3LL * T * T);
  d.add("encoder.mid.attn_1.qkv.bias", PDM_F32, 3LL * T);
  d.add("encoder.mid.attn_1.proj_out.weight", PDM_BF16, 1LL * T * T);
  d.add("encoder.mid.attn_1.proj_out.bias", PDM_F32, T);
  d.add_res("encoder.mid.block_2", T, T);
  d.add("encoder.norm_out.weight", PDM_F32, T);
  d.add("encoder.norm_out.bias", PDM_F32, T);
  d.add("encoder.conv_out.weight", PDM_BF16, 8LL * 9 * T);
  d.add("encoder.conv_out.bias", PDM_F32, 8);
  d.add("quant_conv.weight", PDM_F32, 64);
  d.add("quant_conv.bias", PDM_F32, 8);
  *out = e;
  return PDM_OK;
}

int pdm_encoder_destroy(pdm_encoder* e) {
  delete e;
  return PDM_OK;
}

int pdm_encoder_param_count(const pdm_encoder* e) { return e ? pdm_decoder_param_count(&e->tab) : 0; }

int pdm_encoder_param_info(const pdm_encoder* e, int i, char* name, int len, int* dtype, long long* numel) {
  if (!e) return dfail(PDM_ERR_ARG, "pdm_encoder_param_info: null handle");
  return pdm_decoder_param_info(&e->tab, i, name, len, dtype, numel);
}

int pdm_encoder_set_param(pdm_encoder* e, const char* name, const void* ptr, int dtype, long long numel) {
  if (!e) return dfail(PDM_ERR_ARG, "pdm_encoder_set_param: null handle");
  return pdm_decoder_set_param(&e->tab, name, ptr, dtype, numel);
}

int pdm_encoder_workspace_size(const pdm_encoder* e, int B, size_t* bytes) {
  if (!e || B <= 0 || !bytes) return dfail(PDM_ERR_ARG, "pdm_encoder_workspace_size: bad argument");
  *bytes = elayout(e, B, nullptr).bytes;
  return PDM_OK;
}

int pdm_encoder_encode_moments(pdm_encoder* e, const float* img, float* moments, int B, void* workspace,
                               size_t workspace_bytes, void* stream) {
  if (!e || !img || !moments || B <= 0) return dfail(PDM_ERR_ARG, "pdm_encoder_encode_moments: bad argument");
  const pdm_decoder* d = &e->tab;
  for (auto& n : d->order)
    if (!d->params.at(n).ptr) return dfail(PDM_ERR_STATE, "pdm_encoder: weight not registered: " + n);
  size_t a_bytes = 0;
  DWork w = elayout(e, B, (char*)workspace, &a_bytes);
  // the GEMM addresses the gathered downsample operand with 32-bit buffer offsets
  if (a_bytes >= ((size_t)1 << 31))
    return dfail(PDM_ERR_ARG, "pdm_encoder_encode_moments: batch too large for one launch, encode in chunks");
  if (w.bytes > workspace_bytes) return dfail(PDM_ERR_ARG, "pdm_encoder_encode_moments: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  bool gn_ready = false;
  DCtx c{d, s, &w, &gn_ready};
  D_HIP(hipMemsetAsync(w.zero, 0, 256, s));
  const int T = e->top_ch;
  int res = e->side, cin = e->cfg.ch;
  float* X = w.X;
  float* X2 = w.X2;
  D_HIP(pdm::enc_conv_in_launch(img, d->f("encoder.conv_in.weight"), d->f("encoder.conv_in.bias"), X, B, res, res, cin, s));
  for (int lvl = 0; lvl < e->nlev; ++lvl) {
    const int cout = e->cfg.ch * e->cfg.ch_mult[lvl];
    const std::string p = "encoder.down." + std::to_string(lvl);
    for (int b = 0; b < e->cfg.num_res_blocks; ++b) {
      D_TRY(resblock(c, X, X2, B, res, cin, cout, p + ".block." + std::to_string(b)));
      cin = cout;
    }
    if (lvl != e->nlev - 1) {
      D_TRY(downsample(c, X, X2, B, res, cin, p + ".downsample.conv"));
      res /= 2;
    }
  }
  D_TRY(resblock(c, X, X2, B, res, T, T, "encoder.mid.block_1"));
  D_TRY(attnblock(c, X, B, res, T, "encoder.mid.attn_1"));
  D_TRY(resblock(c, X, X2, B, res, T, T, "encoder.mid.block_2"));
  D_TRY(groupnorm<float>(c, X, B, res * res, T, "encoder.norm_out", w.G, true));
  D_HIP(pdm::enc_tail_launch(w.G, B, res, res, T, d->w("encoder.conv_out.weight"), d->f("encoder.conv_out.bias"),
                             d->f("quant_conv.weight"), d->f("quant_conv.bias"), moments, s));
  return PDM_OK;
}

int pdm_moments_sample(const float* moments, const float* noise, float* z, int B, int C, int hw, float scale,
                       void* stream) {
  if (!moments || !noise || !z || B <= 0 || C <= 0 || hw <= 0)
    return dfail(PDM_ERR_ARG, "pdm_moments_sample: bad argument");
  D_HIP(pdm::moments_sample_launch(moments, noise, z, B, C, hw, scale, (hipStream_t)stream));
  return PDM_OK;
}

// ---- the autoencoder's kernels on caller-owned tensors (parity tests): each entry validates what its kernel assumes
// and then runs the launch function the decoder / encoder run ----------------------------------------------------------
#define V_ARG(cond, msg) \
  do {                   \
    if (!(cond)) return dfail(PDM_ERR_ARG, msg); \
  } while (0)

int pdm_vae_groupnorm(const void* x, int x_dtype, int B, int P, int C, const float* gamma, const float* beta,
                      float eps, int swish, double* part, long long part_elems, int part_ready, void* y, float* stats,
                      void* stream) {
  V_ARG(x && gamma && beta && part && y && stats, "pdm_vae_groupnorm: null argument");
  V_ARG(x_dtype == PDM_F32 || x_dtype == PDM_BF16, "pdm_vae_groupnorm: x must be fp32 or bf16");
  V_ARG(pdm::gn_shape_ok(B, P, C), "pdm_vae_groupnorm: needs B in 1..65535, P > 0, C % 32 == 0 and C <= 1024");
  V_ARG(!part_ready || P % 256 == 0, "pdm_vae_groupnorm: ready-made partials come in whole 256-pixel chunks");
  V_ARG(part_elems >= (long long)B * pdm::gn_chunks(P, C, part_ready != 0) * 64,
        "pdm_vae_groupnorm: partials buffer too small");
  V_ARG(pdm::al16(x) && pdm::al16(y) && ((uintptr_t)part & 7) == 0 && ((uintptr_t)stats & 3) == 0,
        "pdm_vae_groupnorm: x and y must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  if (x_dtype == PDM_F32)
    D_HIP(pdm::gn_launch<float>((const float*)x, B, P, C, gamma, beta, eps, swish != 0, part, part_ready != 0, stats,
                                (bf16*)y, s));
  else
    D_HIP(pdm::gn_launch<bf16>((const bf16*)x, B, P, C, gamma, beta, eps, swish != 0, part, part_ready != 0, stats,
                               (bf16*)y, s));
  return PDM_OK;
}

int pdm_gemm_bf16_gn(const void* A1, int lda1, const void* A2, int lda2, int K1, const void* W, const float* bias, int M,
                     int N, int K, int epi, void* out_bf16, int ldo, float* out_f32, int ldr, int accumulate,
                     double* gn_part, int gn_P, int* fused, void* stream) {
  V_ARG(gn_part && fused && gn_P > 0, "pdm_gemm_bf16_gn: gn_part, fused and a positive gn_P are required");
  pdm::GemmArgs a{};
  a.A1 = (const bf16*)A1; a.lda1 = lda1;
  a.A2 = (const bf16*)A2; a.lda2 = lda2;
  a.K1 = A2 ? K1 : K;
  a.W = (const bf16*)W; a.bias = bias;
  a.M = M; a.N = N; a.K = K;
  a.out_bf16 = (bf16*)out_bf16; a.ldo = ldo;
  a.out_f32 = out_f32; a.ldr = ldr;
  a.accumulate = accumulate;
  bool f = false;
  *fused = 0;
  D_TRY(gemm_gn(a, epi, gn_part, gn_P, (hipStream_t)stream, &f));
  *fused = f ? 1 : 0;
  return PDM_OK;
}

int pdm_gemm_conv3x3_bf16_gn(const void* in, int B, int H, int W, int Cin, int up, const void* Wt, const float* bias,
                             int N, int epi, void* out_bf16, float* out_f32, int accumulate, const void* zero,
                             double* gn_part, int* fused, void* stream) {
  V_ARG(gn_part && fused && zero, "pdm_gemm_conv3x3_bf16_gn: gn_part, fused and the zero page are required");
  V_ARG(B > 0 && H > 0 && W > 0 && (long long)B * H * W <= 0x7fffffffLL, "pdm_gemm_conv3x3_bf16_gn: bad shape");
  pdm::GemmArgs a = conv3_args((const bf16*)in, B, H, W, Cin, up, (const bf16*)Wt, bias, N, (bf16*)out_bf16, out_f32,
                               accumulate, (const bf16*)zero);
  bool f = false;
  *fused = 0;
  D_TRY(gemm_gn(a, epi, gn_part, H * W, (hipStream_t)stream, &f));
  *fused = f ? 1 : 0;
  return PDM_OK;
}

int pdm_vae_softmax_rows(const float* scores, void* probs, long long rows, int n, float scale, void* stream) {
  V_ARG(scores && probs, "pdm_vae_softmax_rows: null argument");
  V_ARG(rows > 0 && rows <= 0x7fffffffLL, "pdm_vae_softmax_rows: bad row count");
  V_ARG(n > 0 && n <= 4096, "pdm_vae_softmax_rows: a row holds 1..4096 columns");
  D_HIP(pdm::softmax_rows_launch(scores, (bf16*)probs, rows, n, scale, (hipStream_t)stream));
  return PDM_OK;
}

int pdm_vae_transpose(const void* src, int ld, int col0, void* dst, int B, int n, int C, void* stream) {
  V_ARG(src && dst, "pdm_vae_transpose: null argument");
  V_ARG(B > 0 && B <= 65535 && n > 0 && n % 32 == 0 && C > 0 && C % 32 == 0 && C / 32 <= 65535,
        "pdm_vae_transpose: needs n % 32 == 0 and C % 32 == 0");
  V_ARG(col0 >= 0 && col0 + C <= ld, "pdm_vae_transpose: the column block must lie inside a row");
  D_HIP(pdm::transpose_launch((const bf16*)src, ld, col0, (bf16*)dst, B, n, C, (hipStream_t)stream));
  return PDM_OK;
}

int pdm_vae_dec_conv_in(const float* z, float scale_factor, const float* pq_w, const float* pq_b, const float* w,
                        const float* bias, float* out, int B, int h, int wd, int Cout, void* stream) {
  V_ARG(z && pq_w && pq_b && w && bias && out, "pdm_vae_dec_conv_in: null argument");
  V_ARG(scale_factor != 0.f, "pdm_vae_dec_conv_in: scale_factor must not be 0");
  V_ARG(B > 0 && B <= 65535 && h > 0 && wd > 0 && Cout > 0, "pdm_vae_dec_conv_in: bad shape");
  V_ARG(wd <= 64, "pdm_vae_dec_conv_in: latent width must be <= 64");
  D_HIP(pdm::dec_conv_in_launch(z, scale_factor, pq_w, pq_b, w, bias, out, B, h, wd, Cout, (hipStream_t)stream));
  return PDM_OK;
}

int pdm_vae_dec_conv_out(const void* g, int B, int H, int W, int C, const void* w, const float* bias, float* img,
                         int out_ch, int force_valu, void* stream) {
  V_ARG(g && w && bias && img, "pdm_vae_dec_conv_out: null argument");
  V_ARG(B > 0 && H > 0 && W > 0 && out_ch >= 1 && out_ch <= 4, "pdm_vae_dec_conv_out: bad shape (out_ch 1..4)");
  V_ARG(C > 0 && C % 8 == 0, "pdm_vae_dec_conv_out: C must be a multiple of 8");
  V_ARG((long long)H * W * C * 2 < 0x7fffffffLL, "pdm_vae_dec_conv_out: one image must stay below 2 GiB");
  V_ARG(pdm::al16(g) && pdm::al16(w) && pdm::al16(img), "pdm_vae_dec_conv_out: g, w and img must be 16-byte aligned");
  V_ARG(pdm::conv_out_mfma(B, H, W, C, force_valu != 0) || 9 * C * 16 <= 65536,
        "pdm_vae_dec_conv_out: the VALU kernel's weights need 9 * C * 16 bytes <= 64 KiB");
  D_HIP(pdm::conv_out_launch((const bf16*)g, B, H, W, C, (const bf16*)w, bias, img, out_ch, force_valu != 0,
                             (hipStream_t)stream));
  return PDM_OK;
}

int pdm_vae_enc_conv_in(const float* img, const float* w, const float* bias, float* out, int B, int H, int W, int C,
                        void* stream) {
  V_ARG(img && w && bias && out, "pdm_vae_enc_conv_in: null argument");
  V_ARG(B > 0 && B <= 65535 && H > 0 && W > 0 && C > 0, "pdm_vae_enc_conv_in: bad shape");
  V_ARG(W <= 512 && C % 16 == 0 && (C + 255) / 256 <= 65535, "pdm_vae_enc_conv_in: needs W <= 512 and C % 16 == 0");
  V_ARG(pdm::al16(out) && pdm::al16(bias), "pdm_vae_enc_conv_in: out and bias must be 16-byte aligned");
  D_HIP(pdm::enc_conv_in_launch(img, w, bias, out, B, H, W, C, (hipStream_t)stream));
  return PDM_OK;
}

int pdm_vae_down_gather(const float* x, void* A, int B, int H, int W, int C, void* stream) {
  V_ARG(x && A, "pdm_vae_down_gather: null argument");
  V_ARG(B > 0 && H > 0 && W > 0 && C > 0 && H % 2 == 0 && W % 2 == 0 && C % 8 == 0,
        "pdm_vae_down_gather: needs even H and W and C % 8 == 0");
  V_ARG((long long)B * (H / 2) * (W / 2) * 9 * (C / 8) <= 0x7fffffffLL * 256, "pdm_vae_down_gather: too many elements");
  V_ARG(pdm::al16(x) && pdm::al16(A), "pdm_vae_down_gather: x and A must be 16-byte aligned");
  D_HIP(pdm::down_gather_launch(x, (bf16*)A, B, H, W, C, (hipStream_t)stream));
  return PDM_OK;
}

int pdm_vae_enc_tail(const void* g, int B, int H, int W, int C, const void* w, const float* cbias, const float* qw,
                     const float* qb, float* moments, void* stream) {
  V_ARG(g && w && cbias && qw && qb && moments, "pdm_vae_enc_tail: null argument");
  V_ARG(B > 0 && H > 0 && W > 0 && C > 0 && C % 32 == 0, "pdm_vae_enc_tail: needs C % 32 == 0");
  V_ARG((long long)B * H * W <= 0x7fffffffLL * 16, "pdm_vae_enc_tail: too many pixels");
  V_ARG(pdm::al16(g) && pdm::al16(w), "pdm_vae_enc_tail: g and w must be 16-byte aligned");
  D_HIP(pdm::enc_tail_launch((const bf16*)g, B, H, W, C, (const bf16*)w, cbias, qw, qb, moments, (hipStream_t)stream));
  return PDM_OK;
}

}  // extern "C"
