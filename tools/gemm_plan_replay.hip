// Host-sanitizer replay of pdm::gemm_plan (CPU only, no GPU touched): gemm.hip's host code compiled into this
// stand-alone program under AddressSanitizer and UBSan, replaying a grid of shapes x epilogues x algos x operand
// options x policies on made-up operand addresses.  Build and run from the repository root:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -fsanitize=address,undefined \
//         tools/gemm_plan_replay.hip -o build/gemm_plan_replay && ASAN_OPTIONS=detect_leaks=0 build/gemm_plan_replay
//
// (the host code is instrumented; the unprefixed -fsanitize links the runtimes and is ignored for the device pass, with
// a warning; leak detection off: the HIP runtime's start-up allocations are not this program's).  Prints the number of
// plans and a checksum of their fields; any sanitizer report fails the run.  About 1.3 million plans in 2 s.
#include "../panopticdiffusionmodels_amd/csrc/gemm.hip"

namespace pdm {   // the launchers gemm.hip's post-passes name (kernels_misc.hip); never called here
hipError_t rowstats_launch(const float*, int, int, int, bf16*, int, float*, int, hipStream_t, unsigned char*, int, unsigned*,
                           int, int) { return hipErrorUnknown; }
hipError_t rowstats_bf16_launch(const bf16*, int, int, int, float*, int, hipStream_t) { return hipErrorUnknown; }
hipError_t rowcopy_launch(float*, int, const float*, int, int, int, int, int, int, hipStream_t, float*, int, const float*, int,
                          int) { return hipErrorUnknown; }
}  // namespace pdm

int main() {
  using namespace pdm;
  const int Ms[] = {1, 255, 256, 4095, 4096, 4133, 65535, 65536, 1100000, 4097 * 256, 8192 * 256};
  const int Ns[] = {4, 96, 100, 120, 128, 132, 256, 264, 1000, 2048, 2056};
  const int Ks[] = {64, 128, 192, 256, 512, 1024, 1152};
  const int algos[] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11};
  char* const base = reinterpret_cast<char*>(uintptr_t(1) << 32);   // made-up, aligned; never dereferenced
  long long n = 0;
  unsigned long long sum = 0;
  for (int M : Ms) for (int N : Ns) for (int K : Ks) for (int epi = 0; epi < 4; ++epi) for (int algo : algos)
    for (int opt = 0; opt < 12; ++opt) {
      GemmArgs p{};
      p.A1 = (const bf16*)base; p.lda1 = K; p.K1 = K; p.W = (const bf16*)(base + (1 << 20));
      p.M = M; p.N = N; p.K = K;
      p.stats_ld = (N + 255) / 256; p.ln_ld = (K + 255) / 256; p.ln_D = K;
      if (epi == EPI_F32) { p.out_f32 = (float*)(base + (2 << 20)) + (opt == 1); p.ldr = N; }
      else { p.out_bf16 = (bf16*)(base + (3 << 20)) + (opt == 1 ? 4 : 0); p.ldo = N + (opt == 2 ? 4 : 0); }
      if (epi == EPI_RES) { p.res_in = p.out_bf16; p.ldri = N; p.accumulate = 1; }
      if (opt == 3 && K >= 128) { p.A2 = (const bf16*)(base + (4 << 20)); p.K1 = K / 128 * 64; p.lda2 = K; }
      if (opt == 4) { p.a_rows_per_group = 100; p.a_group_stride = 120; }
      if (opt == 5) { p.fp8 = 1; p.a_scale = p.w_scale = (const unsigned*)(base + (5 << 20)); p.a_scale_ld = M; p.w_scale_ld = N; }
      if (opt == 6) { p.out_fp8 = (unsigned char*)(base + (6 << 20)); p.ldo8 = N; p.out_scale = (unsigned*)(base + (7 << 20)); p.out_scale_ld = M; if (epi != EPI_F32) p.out_bf16 = nullptr; }
      if (opt == 7) { p.stats_out = (float*)(base + (8 << 20)); p.out2 = (bf16*)(base + (9 << 20)); p.out2_rpg = 100; p.out2_gs = 120; }
      if (opt == 8) { p.sk_flags = (unsigned*)(base + (10 << 20)); p.sk_slab = (float*)(base + (11 << 20)); }
      if (opt == 9) p.batch = 4;
      if (opt == 10 || opt == 11) {
        const int H = 16, W = opt == 10 ? 16 : 1024, C = 64, images = M / (H * W) > 0 ? M / (H * W) : 1;
        p.conv = 1; p.convH = H; p.convW = W; p.convC = C; p.lda1 = C; p.M = images * H * W; p.K = p.K1 = 9 * C;
        p.zero = (const bf16*)(base + (12 << 20));
        p.gn_part = (double*)(base + (13 << 20)); p.gn_P = H * W; p.gn_cpg = N / 32;
      }
      if (gemm_check(p, epi)) continue;
      for (int pol = 0; pol < 4; ++pol) {
        const GemmPolicy g = {algo, pol == 1 ? 2 : 0, 0, pol == 2 ? 1 : 0, 1, pol == 1 ? 24 : 256, pol != 3};
        const GemmPlan pl = gemm_plan(p, epi, g);
        GemmPlan pair{};
        GemmArgs q = p;
        q.M = M / 2 + 4096;
        const bool grouped = !p.conv && gemm_plan_pair(p, q, epi, g, &pair);
        sum = sum * 1000003ull + (unsigned)(pl.error * 7 + pl.family * 131 + pl.kernel + pl.grid_x + pl.split_m1 + pl.writes_gn +
                                            gemm_gn_fusable(p, epi, g) * 3 + grouped * 5 + pair.nt0);
        ++n;
      }
    }
  printf("gemm_plan_replay: %lld plans, checksum %016llx\n", n, sum);
  return n > 2000 ? 0 : 1;
}
