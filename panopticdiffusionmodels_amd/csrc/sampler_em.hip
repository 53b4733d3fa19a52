// Euler-Maruyama step of the reverse SDE / probability-flow ODE (sde.py:243-267) with the noise generated on the
// device, so one captured step serves every step of a trajectory:
//
//   em_step_kernel     final 3x3 conv (optional) + CFG combine (the arithmetic of epilogue_kernel, kernels_misc.hip)
//                      + x' = a x + b e + c z, written to the solver state and to both halves of the model input.
//                      (a, b, c) come from row k of a device table, k from a device-resident step counter, z from
//                      Philox4x32-10 keyed on (seed; element quad, step, global sample index).
//   em_advance_kernel  one thread block launched behind it on the same stream: writes the next step's net time into
//                      the [rows] time buffer the next forward reads, then counter = k + 1.
//
// The counter scheme: every block of em_step_kernel only READS the counter; the single writer is the trailing
// em_advance launch, which by stream order starts after the last block of the step kernel has finished and
// finishes before the next forward (and the next step kernel) starts.  So all blocks of a step see one value of k
// and no block can advance it under another; nothing but stream order is relied on (no atomics, no flags).
// The time buffer is written by the same trailing launch: the forward that read it has finished by then.
//
// Noise (host model: panopticdiffusionmodels_amd/philox.py):
//   key = (seed lo, seed hi), counter = (quad within the sample, step, sample lo, sample hi); element o of a sample
//   takes word o & 3 of quad o >> 2; u = ((r >> 8) + 0.5) 2^-24; Box-Muller on the word pairs (0, 1) and (2, 3).
// A thread owns one quad (4 consecutive elements of one sample): one Philox call, two Box-Muller pairs.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/pdm.h"
#include "pdm_kernels.h"

namespace pdm {
namespace {

struct u32x4 {
  uint32_t v[4];
};

__device__ __forceinline__ u32x4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                               uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0;
    c1 = l1;
    c2 = h0 ^ c3 ^ k1;
    c3 = l0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return u32x4{{c0, c1, c2, c3}};
}

__device__ __forceinline__ u32x4 noise_words(unsigned long long seed, unsigned long long sample, uint32_t step,
                                             uint32_t quad) {
  return philox4x32_10(quad, step, (uint32_t)sample, (uint32_t)(sample >> 32), (uint32_t)seed,
                       (uint32_t)(seed >> 32));
}

// u = (m + 0.5) 2^-24 with m = r >> 8 is a 25-bit number: exact in fp32 only for m < 2^23.  Above that its
// complement d = 1 - u = ((2^24 - 1 - m) + 0.5) 2^-24 is exact instead, so ln u and the angle are taken from d
// there (log1p(-d); sin 2 pi u = -sin 2 pi d, cos 2 pi u = cos 2 pi d).  Rounding u itself to fp32 near 1 would
// cost 3e-6 absolutely on small radii (measured).
__device__ __forceinline__ float unit_lo(uint32_t m) { return ((float)m + 0.5f) * 0x1p-24f; }

// cos / sin (2 pi u) as cospi / sinpi (2 u): the argument scaling is exact
__device__ __forceinline__ void box_muller(uint32_t ra, uint32_t rb, float& na, float& nb) {
  const uint32_t ma = ra >> 8, mb = rb >> 8;
  const float lnu = ma < (1u << 23) ? logf(unit_lo(ma)) : log1pf(-unit_lo(0xFFFFFFu - ma));
  const float rad = sqrtf(-2.0f * lnu);
  float s, c;
  if (mb < (1u << 23)) {
    sincospif(2.0f * unit_lo(mb), &s, &c);
  } else {
    sincospif(2.0f * unit_lo(0xFFFFFFu - mb), &s, &c);
    s = -s;
  }
  na = rad * c;
  nb = rad * s;
}

__device__ __forceinline__ void normals4(const u32x4& r, float (&z)[4]) {
  box_muller(r.v[0], r.v[1], z[0], z[1]);
  box_muller(r.v[2], r.v[3], z[2], z[3]);
}

// final_layer conv3x3 (libs/uvit.py:183,229), the arithmetic of conv3x3_at in kernels_misc.hip (restated here so
// that translation unit's code object stays as it is)
__device__ __forceinline__ float em_conv3x3_at(const float* img, const float* w, const float* bias, int C, int H,
                                               int W, int c, int y, int x) {
  float acc = bias[c];
  for (int ci = 0; ci < C; ++ci) {
    const float* ip = img + (size_t)ci * H * W;
    const float* wp = w + ((size_t)c * C + ci) * 9;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const int yy = y + ky - 1;
      if (yy < 0 || yy >= H) continue;
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int xx = x + kx - 1;
        if (xx < 0 || xx >= W) continue;
        acc = fmaf(wp[ky * 3 + kx], ip[(size_t)yy * W + xx], acc);
      }
    }
  }
  return acc;
}

struct EmArgs {
  const float* pre;
  const float* w; const float* bias;
  int B, C, H, W;
  int has_uncond; float cfg_scale;
  float* x; float* xin;
  const float* table; int steps;
  const int* counter;
  unsigned long long seed, sample_offset;
  const unsigned long long* offset_dev;
};

__global__ __launch_bounds__(256) void em_step_kernel(EmArgs p) {
  const int k = *p.counter;   // read-only here: em_advance_kernel is the only writer (file comment)
  if (k < 0 || k >= p.steps) return;   // a launch past the end of the table leaves everything as it is
  const float a = p.table[4 * k + 1], bc = p.table[4 * k + 2], cz = p.table[4 * k + 3];
  const int hw = p.H * p.W;
  const long long per = (long long)p.C * hw;
  const long long nq = (per + 3) >> 2;
  const long long total = nq * p.B;
  // global index of sample 0: the by-value part plus the device-resident part (a captured step serves any batch
  // position: the caller rewrites *offset_dev between replays)
  const unsigned long long s0 = p.sample_offset + (p.offset_dev ? *p.offset_dev : 0ull);
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int b = (int)(i / nq);
    const long long q = i % nq;
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    if (cz != 0.f) normals4(noise_words(p.seed, s0 + (unsigned long long)b, (uint32_t)k, (uint32_t)q), z);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long long r = 4 * q + j;
      if (r >= per) break;
      const int c = (int)(r / hw), yx = (int)(r % hw);
      const int y = yx / p.W, x = yx % p.W;
      float v;
      if (p.w) v = em_conv3x3_at(p.pre + (size_t)b * per, p.w, p.bias, p.C, p.H, p.W, c, y, x);
      else v = p.pre[(size_t)b * per + r];
      if (p.has_uncond) {
        float u;
        if (p.w) u = em_conv3x3_at(p.pre + (size_t)(b + p.B) * per, p.w, p.bias, p.C, p.H, p.W, c, y, x);
        else u = p.pre[(size_t)(b + p.B) * per + r];
        v = v + p.cfg_scale * (v - u);
      }
      const size_t e = (size_t)b * per + r;
      const float xn = a * p.x[e] + bc * v + cz * z[j];
      p.x[e] = xn;
      p.xin[e] = xn;
      if (p.has_uncond) p.xin[(size_t)p.B * per + e] = xn;
    }
  }
}

// the step's only writer of the counter and the time buffer; launched alone behind em_step_kernel
__global__ __launch_bounds__(256) void em_advance_kernel(const float* table, int steps, int* counter, float* t_next,
                                                         int rows) {
  const int k = *counter;
  if (k < 0 || k >= steps) return;
  if (k + 1 < steps) {
    const float t = table[4 * (k + 1)];
    for (int r = threadIdx.x; r < rows; r += 256) t_next[r] = t;
  }
  __syncthreads();   // every thread has read k
  if (threadIdx.x == 0) *counter = k + 1;
}

__global__ __launch_bounds__(256) void philox_fill_kernel(float* out, uint32_t* raw, int B, long long per,
                                                          unsigned long long seed, unsigned long long sample_offset,
                                                          uint32_t step) {
  const long long nq = (per + 3) >> 2;
  const long long total = nq * B;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int b = (int)(i / nq);
    const long long q = i % nq;
    const u32x4 r = noise_words(seed, sample_offset + (unsigned long long)b, step, (uint32_t)q);
    float z[4];
    if (out) normals4(r, z);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long long o = 4 * q + j;
      if (o >= per) break;
      if (out) out[(size_t)b * per + o] = z[j];
      if (raw) raw[(size_t)b * per + o] = r.v[j];
    }
  }
}

int em_grid(long long n) {
  long long g = (n + 255) / 256;
  if (g > 8192) g = 8192;
  if (g < 1) g = 1;
  return (int)g;
}

const char* em_check(const pdm_em_step_args& a) {
  if (!a.pre || !a.x || !a.xin) return "em_step: null input / state / model input";
  if (a.B <= 0 || a.C <= 0 || a.H <= 0 || a.W <= 0) return "em_step: B, C, H, W must be positive";
  if (a.conv_w && !a.conv_b) return "em_step: conv bias missing";
  if (!a.table || a.steps <= 0) return "em_step: coefficient table [steps, 4] missing or steps <= 0";
  if (!a.counter || !a.t_next) return "em_step: null step counter / time buffer";
  if ((long long)a.C * a.H * a.W > (1ll << 33)) return "em_step: sample too large for a 32-bit quad index";
  return nullptr;
}

int philox_fill(float* out, uint32_t* raw, int B, int per_sample, unsigned long long seed,
                unsigned long long sample_offset, int step, void* stream, const char* who) {
  if ((!out && !raw) || B <= 0 || per_sample <= 0 || step < 0)
    return set_error(PDM_ERR_ARG, std::string(who) + ": bad argument");
  const long long nq = ((long long)per_sample + 3) >> 2;
  hipLaunchKernelGGL(philox_fill_kernel, dim3(em_grid(nq * B)), dim3(256), 0, (hipStream_t)stream, out, raw, B,
                     (long long)per_sample, seed, sample_offset, (uint32_t)step);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? PDM_OK : set_error(PDM_ERR_HIP, hipGetErrorString(e));
}

}  // namespace
}  // namespace pdm

extern "C" {

int pdm_em_step(const pdm_em_step_args* a, void* stream) {
  if (!a) return pdm::set_error(PDM_ERR_ARG, "pdm_em_step: null args");
  if (const char* m = pdm::em_check(*a)) return pdm::set_error(PDM_ERR_ARG, m);
  pdm::EmArgs p{};
  p.pre = a->pre; p.w = a->conv_w; p.bias = a->conv_b;
  p.B = a->B; p.C = a->C; p.H = a->H; p.W = a->W;
  p.has_uncond = a->has_uncond; p.cfg_scale = a->cfg_scale;
  p.x = a->x; p.xin = a->xin;
  p.table = a->table; p.steps = a->steps; p.counter = a->counter;
  p.seed = a->seed; p.sample_offset = a->sample_offset; p.offset_dev = a->sample_offset_dev;
  const long long nq = ((long long)a->C * a->H * a->W + 3) >> 2;
  hipLaunchKernelGGL(pdm::em_step_kernel, dim3(pdm::em_grid(nq * a->B)), dim3(256), 0, (hipStream_t)stream, p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return pdm::set_error(PDM_ERR_HIP, hipGetErrorString(e));
  hipLaunchKernelGGL(pdm::em_advance_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a->table, a->steps,
                     a->counter, a->t_next, a->has_uncond ? 2 * a->B : a->B);
  e = hipGetLastError();
  return e == hipSuccess ? PDM_OK : pdm::set_error(PDM_ERR_HIP, hipGetErrorString(e));
}

int pdm_philox_normal(float* out, int B, int per_sample, unsigned long long seed, unsigned long long sample_offset,
                      int step, void* stream) {
  return pdm::philox_fill(out, nullptr, B, per_sample, seed, sample_offset, step, stream, "pdm_philox_normal");
}

int pdm_philox_raw(uint32_t* out, int B, int per_sample, unsigned long long seed, unsigned long long sample_offset,
                   int step, void* stream) {
  return pdm::philox_fill(nullptr, out, B, per_sample, seed, sample_offset, step, stream, "pdm_philox_raw");
}

}  // extern "C"
