// C ABI of libpdm (include/pdm.h) and the U-ViT forward drivers.
//
// The drivers restate the layer loops of libs/uvit.py:201-230 and libs/uvit_t2i.py:378-525 as a fixed
// sequence of stream-ordered kernel launches over a caller-owned workspace: no allocation, no host sync,
// so a whole forward (or a whole sampler step) can be captured into a HIP graph.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/pdm.h"
#include "pdm_kernels.h"

using pdm::bf16;

namespace {

thread_local std::string g_err;
bool g_sk_standalone = false;       // pdm_set_gemm_sk bit 2: standalone pdm_gemm calls take stream-K (library state)
constexpr int SK_LAUNCHES = 512;    // stream-K flag blocks per forward workspace (GEMM launches of one forward)

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

}  // namespace

namespace pdm {
int set_error(int code, const std::string& msg) { return fail(code, msg); }
}  // namespace pdm

namespace {

#define PDM_HIP(call)                                                                   \
  do {                                                                                  \
    hipError_t e_ = (call);                                                             \
    if (e_ != hipSuccess) return fail(PDM_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
  } while (0)

#define PDM_TRY(x)           \
  do {                       \
    int r_ = (x);            \
    if (r_) return r_;       \
  } while (0)

#define PDM_CHECK(msg_expr)                          \
  do {                                               \
    const char* m_ = (msg_expr);                     \
    if (m_) return fail(PDM_ERR_ARG, m_);            \
  } while (0)

size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

struct ParamSpec {
  int dtype;
  long long numel;
  const void* ptr = nullptr;
};

// Registered weights resolved to pointers (pdm_uvit::resolve), so a forward builds no key and searches no map.
// One Linear: weight, bias (a LayerNorm consumer's ln_bias) and, where registered, ln_colsum, the MXFP8 weight's
// "_scale" and the consumer's ln_gcol; null where the network has none.
struct LinW {
  const bf16* w = nullptr;
  const float* bias = nullptr;
  const float* colsum = nullptr;
  const unsigned* scale = nullptr;
  const bf16* gcol = nullptr;
};
struct BlockW {
  LinW qkv, proj, fc1, fc2, skip;   // skip.w null: no long skip
};
// One layer of the in / mid / out walk (libs/uvit.py:213-222): its image block, its mask block and zero-conv (a
// `separate` panoptic net, libs/uvit_t2i.py:411-472), and the long-skip wiring, fixed at create time.
struct Layer {
  BlockW img, mask;
  LinW zc;
  int keep = -1;        // in-block i: its output is kept in long-skip slot i
  int skip_from = -1;   // out-block with a long skip: the slot its skip_linear reads
  bool last = false;    // the last out-block
};

}  // namespace

struct pdm_uvit {
  pdm_uvit_cfg cfg;
  int D, H, Dh, Hid, C, p, n_patch, extras, Lx, Lm, P, P_pad, K, PK, PK_pad, depth, nhalf;
  std::vector<std::string> order;
  std::map<std::string, ParamSpec> params;
  // the resolved table: rebuilt by check_ready after pdm_uvit_set_param (dirty)
  bool dirty = true;
  std::vector<Layer> layers;
  LinW ctx_embed, head, head_mask;
  const float *pos = nullptr, *pos_mask = nullptr, *patch_w = nullptr, *patch_b = nullptr, *mask_w = nullptr,
              *mask_b = nullptr, *label_emb = nullptr, *norm_w = nullptr, *norm_b = nullptr;
  // profiling hook: events around every GEMM launch of the last forward (bench roofline)
  mutable std::vector<hipEvent_t> prof_ev;
  mutable std::vector<double> prof_flops;
  mutable int prof_n = 0;
  mutable bool prof_on = false;

  void add(const std::string& name, int dtype, long long numel) {
    order.push_back(name);
    params[name] = ParamSpec{dtype, numel, nullptr};
  }
  const void* ptr(const std::string& name) const {
    auto it = params.find(name);
    return it == params.end() ? nullptr : it->second.ptr;
  }
  const float* f(const std::string& name) const { return static_cast<const float*>(ptr(name)); }
  const bf16* w(const std::string& name) const { return static_cast<const bf16*>(ptr(name)); }

  // norm1 / norm2 are folded into the next Linear (fused LayerNorm, see GemmArgs): the registered
  // attn.qkv.weight / mlp.fc1.weight are W * diag(norm.weight) in bf16, ln_colsum their row sums and ln_bias
  // W norm.bias (+ the Linear's own bias), both fp32 (include/pdm.h)
  // the residual stream is bf16 (cfg.residual_fp32 == 0)
  bool res16() const { return !cfg.residual_fp32; }
  // the joint image+mask sequence (libs/uvit_t2i.py with enable_panoptic and separate=False): one block stack
  bool joint() const { return cfg.t2i && cfg.enable_panoptic && !cfg.separate; }
  // block Linear `bit` (0 qkv, 1 proj, 2 fc1, 3 fc2) runs in MXFP8 (cfg.fp8 / cfg.fp8_linears)
  bool f8(int bit) const { return cfg.fp8 && (((cfg.fp8_linears ? cfg.fp8_linears : 0xF) >> bit) & 1); }
  // a block Linear's weight [N][K]: bf16, or (MXFP8) e4m3 bytes + "<key>_scale" E8M0 dwords [K/128][N]; an MXFP8
  // LayerNorm consumer (qkv, fc1) also takes the bf16 hi / lo group sums "<lin>.ln_gcol" [N][16]
  void add_lin(const std::string& key, long long N, long long K, int bit, bool ln) {
    if (f8(bit)) {
      add(key, PDM_FP8, N * K);
      add(key + "_scale", PDM_E8M0, K / 128 * N);
      if (ln) add(key.substr(0, key.size() - 7) + ".ln_gcol", PDM_BF16, N * 16);
    } else {
      add(key, PDM_BF16, N * K);
    }
  }
  void add_block(const std::string& pre, bool skip) {
    add_lin(pre + ".attn.qkv.weight", 3LL * D, D, 0, true);
    add(pre + ".attn.qkv.ln_colsum", PDM_F32, 3LL * D);
    add(pre + ".attn.qkv.ln_bias", PDM_F32, 3LL * D);
    add_lin(pre + ".attn.proj.weight", D, D, 1, false);
    add(pre + ".attn.proj.bias", PDM_F32, D);
    add_lin(pre + ".mlp.fc1.weight", Hid, D, 2, true);
    add(pre + ".mlp.fc1.ln_colsum", PDM_F32, Hid);
    add(pre + ".mlp.fc1.ln_bias", PDM_F32, Hid);
    add_lin(pre + ".mlp.fc2.weight", D, Hid, 3, false);
    add(pre + ".mlp.fc2.bias", PDM_F32, D);
    if (skip) {
      add(pre + ".skip_linear.weight", PDM_BF16, 2LL * D * D);   // bf16 also in an MXFP8 net (run_block)
      add(pre + ".skip_linear.bias", PDM_F32, D);
    }
  }
  // state_dict prefix of layer l's block: in_blocks.i, mid_block, out_blocks.i (+ "_mask": the mask stream's)
  std::string block_name(int l, const char* sfx) const {
    if (l == nhalf) return std::string("mid_block") + sfx;
    return (l < nhalf ? "in_blocks" : "out_blocks") + std::string(sfx) + "." + std::to_string(l < nhalf ? l : l - nhalf - 1);
  }
  static std::string zc_name(int l) { return "zero_convs." + std::to_string(2 * l + 1) + ".conv"; }
  void add_stack(const char* sfx) {
    for (int l = 0; l <= 2 * nhalf; ++l) add_block(block_name(l, sfx), l > nhalf && cfg.skip);
  }
  void resolve() {
    auto lin = [&](const std::string& p, bool ln = false) {
      LinW l;
      l.w = w(p + ".weight");
      l.bias = f(p + (ln ? ".ln_bias" : ".bias"));
      l.colsum = f(p + ".ln_colsum");
      l.scale = static_cast<const unsigned*>(ptr(p + ".weight_scale"));
      l.gcol = w(p + ".ln_gcol");
      return l;
    };
    auto block = [&](const std::string& pre) {
      return BlockW{lin(pre + ".attn.qkv", true), lin(pre + ".attn.proj"), lin(pre + ".mlp.fc1", true),
                    lin(pre + ".mlp.fc2"), lin(pre + ".skip_linear")};
    };
    for (int l = 0; l < (int)layers.size(); ++l) {
      layers[l].img = block(block_name(l, ""));
      layers[l].mask = block(block_name(l, "_mask"));
      layers[l].zc = lin(zc_name(l));
    }
    ctx_embed = lin("context_embed");
    head = lin("decoder_pred");
    head_mask = lin("decoder_pred_mask");
    pos = f("pos_embed"); pos_mask = f("pos_embed_mask");
    patch_w = f("patch_embed.proj.weight"); patch_b = f("patch_embed.proj.bias");
    mask_w = f("mask_embed.proj.weight"); mask_b = f("mask_embed.proj.bias");
    label_emb = f("label_emb.weight");
    norm_w = f("norm.weight"); norm_b = f("norm.bias");
    dirty = false;
  }
};

namespace {

// ------------------------------------------------------------------------------------------------
// An MXFP8 matrix in the GemmArgs operand layout: e4m3 rows q [rows][ld] (bytes) and E8M0 scale dwords
// s [K/128][sld].  cols(k0) is the same rows from column k0 on (k0 % 128 == 0).
struct Q8 {
  unsigned char* q = nullptr;
  int ld = 0;
  unsigned* s = nullptr;
  int sld = 0;
  Q8 cols(int k0) const { return Q8{q + k0, ld, s + (size_t)(k0 / 128) * sld, sld}; }
};

// workspace layout
struct Workspace {
  float* X;     // [rows*Lx, D] residual stream (image); a joint net (t2i, separate=False): [rows*Lm, D] here, in XB / SK
  bf16* XB;     // [rows*Lx, D] bf16 copy of x (qkv / skip_linear A operand)
  bf16* XT;     // [rows*Lmax, D] bf16 copy of the block-internal x (after skip_linear / attention)
  float* ST;    // [rows*Lmax, T] (sum, M2) LayerNorm partials of x at block entry / exit, T = ceil(D/256)
  float* STT;   // [rows*Lmax, T] partials of the block-internal x
  bf16* QKV;    // [rows*Lmax, 3D]
  bf16* ATT;    // [rows*Lmax, D]
  bf16* MLP;    // [rows*Lmax, Hid]
  bf16* SK;     // [nhalf][rows*Lx, D] long-skip activations (image)
  bf16* HEADIN; // [rows*n_patch, D]; a joint net: [rows*2*n_patch, D] (image rows, then mask rows, per sample)
  // t2i
  float* CTXF;  // [rows*n_ctx, D] embedded context (fp32)
  bf16* CTXB;   // [rows*n_ctx, clip_dim] bf16 context
  float* MX;    // [rows*Lm, D] mask stream
  bf16* MXB;    // [rows*Lm, D] bf16 copy of the mask-stream block output
  bf16* MXIN;   // [rows*Lm, D] bf16 copy of the mask-stream block input (qkv / skip_linear operand)
  bf16* MB;     // [rows*Lm, D] bf16 mask-stream block input (bf16 residual stream: MX is then only assembly scratch)
  bf16* SKM;    // [nhalf][rows*Lm, D]
  float* STM;   // [rows*Lm, T] LayerNorm partials of the mask stream
  // t2i on the bf16 stream: the image block's own scratch, so it runs in lockstep with the mask block of its layer
  // (every block Linear of the pair one grouped launch, run_block on two streams)
  bf16 *XT2, *QKV2, *ATT2, *MLP2;
  float* STT2;
  // fp8 forward (cfg.fp8): MXFP8 operands of the block Linears, e4m3 rows + E8M0 scale dwords [K/128][rows*Lx]
  Q8 xq;             // block input x (from the token assembly row pass)                 [rows*Lx, D]
  Q8 xtq;            // block-internal x (skip_linear / proj epilogues: qkv / fc1 operand) [rows*Lx, D]
  Q8 atq;            // attention output (proj operand)                                  [rows*Lx, D]
  Q8 mlq;            // GELU(fc1) (fc2 operand)                                          [rows*Lx, Hid]
  size_t bytes;
};

Workspace layout(const pdm_uvit* h, int rows, char* base) {
  Workspace w{};
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + off : nullptr;
    off = align_up(off + bytes, 256);
    return p;
  };
  const size_t D = h->D;
  // a joint net runs its one stack over [time, context, image patches, mask patches]: every buffer of the single
  // stream holds Lm rows per sample, the head input both patch halves, and there is no mask stream
  const bool joint = h->joint();
  const size_t Mx = (size_t)rows * (joint ? h->Lm : h->Lx);
  const bool mask = h->cfg.t2i && h->cfg.separate && h->cfg.enable_panoptic;
  const size_t Mm = mask ? (size_t)rows * h->Lm : 0;
  const size_t Mmax = Mx > Mm ? Mx : Mm;
  const size_t T = (D + 255) / 256;
  const bool f8 = h->cfg.fp8 != 0;   // MXFP8 operands replace XT / MLP; XB / SK stay (bf16 skip_linear)
  w.X = (float*)take(Mx * D * 4);
  w.XB = (bf16*)take(Mx * D * 2);
  if (!f8 || !h->f8(2) || h->res16()) w.XT = (bf16*)take(Mmax * D * 2);   // (fp8: bf16 fc1 operand / bf16 stream)
  w.ST = (float*)take(Mmax * T * 8);
  w.STT = (float*)take(Mmax * T * 8);
  w.QKV = (bf16*)take(Mmax * 3 * D * 2);
  w.ATT = (bf16*)take(Mmax * D * 2);
  if (!f8) w.MLP = (bf16*)take(Mmax * h->Hid * 2);
  w.SK = (bf16*)take((size_t)h->nhalf * Mx * D * 2);
  w.HEADIN = (bf16*)take((size_t)rows * (joint ? 2 : 1) * h->n_patch * D * 2);
  if (f8) {
    auto q8 = [&](size_t K) {
      Q8 r;
      r.q = (unsigned char*)take(Mx * K);
      r.ld = (int)K;
      r.s = (unsigned*)take(K / 128 * Mx * 4);
      r.sld = (int)Mx;
      return r;
    };
    w.xq = q8(D);
    w.xtq = q8(D);   // skip_linear output (qkv operand), and proj output (fc1 operand) when fc1 is MXFP8
    w.atq = q8(D);
    w.mlq = q8(h->Hid);
  }
  if (h->cfg.t2i) {
    w.CTXF = (float*)take((size_t)rows * h->cfg.num_clip_token * D * 4);
    w.CTXB = (bf16*)take((size_t)rows * h->cfg.num_clip_token * h->cfg.clip_dim * 2);
  }
  if (mask) {
    if (h->res16()) w.MB = (bf16*)take(Mm * D * 2);
    w.MX = (float*)take(Mm * D * 4);
    w.MXB = (bf16*)take(Mm * D * 2);
    w.MXIN = (bf16*)take(Mm * D * 2);
    w.STM = (float*)take(Mm * T * 8);
    w.SKM = (bf16*)take((size_t)h->nhalf * Mm * D * 2);
    if (h->res16() && !f8) {
      w.XT2 = (bf16*)take(Mx * D * 2);
      w.STT2 = (float*)take(Mx * T * 8);
      w.QKV2 = (bf16*)take(Mx * 3 * D * 2);
      w.ATT2 = (bf16*)take(Mx * D * 2);
      w.MLP2 = (bf16*)take(Mx * h->Hid * 2);
    }
  }
  w.bytes = off;   // (stream-K's flags and slab are library-owned per stream: sk_state)
  return w;
}

// ------------------------------------------------------------------------------------------------
struct Ctx {
  const pdm_uvit* h;
  hipStream_t s;
  // stream-K state of this forward (null: whole-tile GEMMs): flag blocks handed out one per GEMM launch
  unsigned* skf = nullptr;
  float* sks = nullptr;
  int* skn = nullptr;
  int sk_used = 0;   // what skn counts in (begin_forward)
};

// Stream-K state of the persistent GEMM (pdm::GemmArgs::sk_flags / sk_slab): SK_RING blocks of SK_FLAG_WORDS flag
// words (one block per GEMM launch) + one 64 MiB fp32 accumulator slab reused launch after launch in stream order.
// Owned by the library, one state per (device, stream), allocated on first use -- stream-K is off by default, so no
// forward workspace carries its 64 MiB, every device has its own (a process driving several GPUs), and
// concurrent streams (the sampling lanes) never share a slab.  Never allocated inside a stream capture: a forward
// captured on a stream without a state keeps whole tiles.
constexpr int SK_RING = 4096;
struct SkState {
  unsigned* flags = nullptr;
  float* slab = nullptr;
  int next = 0;   // next free flag block (host order of the launches on this stream); blocks past it are zero
};
static std::mutex g_sk_mu;
static std::map<std::pair<int, hipStream_t>, SkState> g_sk_state;

static int sk_state(hipStream_t s, SkState** out) {
  *out = nullptr;
  int dev = 0;
  PDM_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(g_sk_mu);
  auto it = g_sk_state.find({dev, s});
  if (it == g_sk_state.end()) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    PDM_HIP(hipStreamIsCapturing(s, &cs));
    if (cs != hipStreamCaptureStatusNone) return PDM_OK;   // no allocation inside a capture: whole tiles
    SkState st;
    PDM_HIP(hipMalloc(&st.flags, (size_t)SK_RING * pdm::SK_FLAG_WORDS * 4));
    PDM_HIP(hipMalloc(&st.slab, (size_t)pdm::SK_SLAB_BYTES));
    PDM_HIP(hipMemsetAsync(st.flags, 0, (size_t)SK_RING * pdm::SK_FLAG_WORDS * 4, s));
    it = g_sk_state.emplace(std::make_pair(dev, s), st).first;
  }
  *out = &it->second;
  return PDM_OK;
}

// a forward's stream-K state: SK_LAUNCHES flag blocks of the stream's ring, zeroed on the stream first (one memset
// node in a captured graph, so every replay starts from zeroed flags); none while the policy is off (a graph
// captured then keeps whole tiles)
int sk_begin(Ctx& c, int* counter) {
  *counter = 0;
  if (pdm::gemm_get_sk() == 0) return PDM_OK;
  SkState* st = nullptr;
  PDM_TRY(sk_state(c.s, &st));
  if (!st) return PDM_OK;
  if (st->next + SK_LAUNCHES > SK_RING) {   // wrap: the whole ring zeroed, so blocks past `next` stay clean
    PDM_HIP(hipMemsetAsync(st->flags, 0, (size_t)SK_RING * pdm::SK_FLAG_WORDS * 4, c.s));
    st->next = 0;
  }
  unsigned* f = st->flags + (size_t)st->next * pdm::SK_FLAG_WORDS;
  st->next += SK_LAUNCHES;
  PDM_HIP(hipMemsetAsync(f, 0, (size_t)SK_LAUNCHES * pdm::SK_FLAG_WORDS * 4, c.s));
  c.skf = f;
  c.sks = st->slab;
  c.skn = counter;
  return PDM_OK;
}

// checked launch + the profiling hook (HIP events around every GEMM of the forward)
int launch_gemm(const Ctx& c, const pdm::GemmArgs& a, int epi) {
  PDM_CHECK(pdm::gemm_check(a, epi));
  const pdm_uvit* h = c.h;
  const bool prof = h->prof_on && 2 * (h->prof_n + 1) <= (int)h->prof_ev.size();
  pdm::GemmArgs b = a;
  if (c.skf && *c.skn < SK_LAUNCHES) {   // this launch's own zeroed flag block (used only if it takes stream-K)
    b.sk_flags = c.skf + (size_t)(*c.skn)++ * pdm::SK_FLAG_WORDS;
    b.sk_slab = c.sks;
  }
  if (prof) PDM_HIP(hipEventRecord(h->prof_ev[2 * h->prof_n], c.s));
  PDM_HIP(pdm::gemm_launch(b, epi, c.s));
  if (prof) {
    PDM_HIP(hipEventRecord(h->prof_ev[2 * h->prof_n + 1], c.s));
    h->prof_flops[h->prof_n] = 2.0 * a.M * a.N * a.K;
    ++h->prof_n;
  }
  return PDM_OK;
}

// two GEMMs as one grouped launch where the kernel takes both (pdm::gemm_launch_pair), with the profiling hook
// counting the pair as one launch of their summed FLOPs
int launch_gemm_pair(const Ctx& c, const pdm::GemmArgs& a, const pdm::GemmArgs& b, int epi) {
  PDM_CHECK(pdm::gemm_check(a, epi));
  PDM_CHECK(pdm::gemm_check(b, epi));
  const pdm_uvit* h = c.h;
  // not grouped: two launches, each with its own profiling entry (the roofline counts launches)
  if (!pdm::gemm_pair_groups(a, b, epi)) {
    const int r = launch_gemm(c, a, epi);
    return r != PDM_OK ? r : launch_gemm(c, b, epi);
  }
  const bool prof = h->prof_on && 2 * (h->prof_n + 1) <= (int)h->prof_ev.size();
  if (prof) PDM_HIP(hipEventRecord(h->prof_ev[2 * h->prof_n], c.s));
  PDM_HIP(pdm::gemm_launch_pair(a, b, epi, c.s));
  if (prof) {
    PDM_HIP(hipEventRecord(h->prof_ev[2 * h->prof_n + 1], c.s));
    h->prof_flops[h->prof_n] = 2.0 * a.M * a.N * a.K + 2.0 * b.M * b.N * b.K;
    ++h->prof_n;
  }
  return PDM_OK;
}

// How a forward runs its blocks ("forward orchestration"):
//   r16: the residual stream x is bf16 (cfg.residual_fp32 == 0): the residual Linears take EPI_RES, out = bf16(A W^T
//        + bias (+ x)), and x lives in bf16 buffers; else x is fp32 in X, they take EPI_F32 (X (+)= ...) and leave a
//        bf16 copy for the next bf16 operand
//   f8:  which block Linears are MXFP8, bit 0 qkv, 1 proj, 2 fc1, 3 fc2 (0: none; pdm_uvit_create admits 0xF and
//        0xB, so qkv, proj and fc2 go together)
struct Mode {
  bool r16;
  int f8;
};
Mode mode_of(const pdm_uvit* h) {
  return Mode{h->res16(), h->cfg.fp8 ? (h->cfg.fp8_linears ? h->cfg.fp8_linears : 0xF) : 0};
}

// GemmArgs of a LayerNorm-consuming block Linear (qkv, fc1; norm1 / norm2 folded into the weight, see pdm_uvit):
// out = epi(LN(x) W^T + bias) from bf16 x [M][K] and its partials st_in
pdm::GemmArgs ln_lin(const pdm_uvit* h, const bf16* A, const LinW& lw, int M, int N, int K, bf16* out,
                     const float* st_in) {
  pdm::GemmArgs a{};
  const int T = (h->D + 255) / 256;
  a.ln_stats = st_in; a.ln_ld = T; a.ln_D = K; a.ln_eps = 1e-5f; a.ln_colsum = lw.colsum; a.stats_ld = T;
  a.A1 = A; a.lda1 = K; a.K1 = K;
  a.W = lw.w; a.bias = lw.bias;
  a.M = M; a.N = N; a.K = K;
  a.out_bf16 = out; a.ldo = N;
  return a;
}

// GemmArgs of a residual-producing Linear (skip_linear, proj, fc2, the t2i injection): D output columns and their
// LayerNorm partials in st_out.  With A2, the second split-K operand, it is skip_linear(cat([x, skip], -1)), whose
// output replaces x; every other one adds to x.
//   bf16 stream (EPI_RES): out = bf16(A W^T + bias (+ res)); res may alias out
//   fp32 stream (EPI_F32): X (+)= A W^T + bias, and out (may be null) takes bf16 of the new X
pdm::GemmArgs res_lin(const pdm_uvit* h, Mode m, const bf16* A, int lda, const bf16* A2, const LinW& lw, int M, int K,
                      float* X, const bf16* res, bf16* out, float* st_out) {
  pdm::GemmArgs a{};
  const int D = h->D, T = (D + 255) / 256;
  a.A1 = A; a.lda1 = lda;
  a.A2 = A2; a.lda2 = A2 ? D : 0;
  a.K1 = A2 ? D : K;
  a.W = lw.w; a.bias = lw.bias;
  a.M = M; a.N = D; a.K = K;
  a.out_bf16 = out; a.ldo = D;
  a.accumulate = A2 ? 0 : 1;
  a.stats_out = st_out; a.stats_ld = T;
  if (m.r16) {
    a.res_in = res; a.ldri = D;
  } else {
    a.out_f32 = X; a.ldr = D;
    // the bf16 Linears of the fp32 stream have always carried these, though none consumes a LayerNorm
    if (!m.f8) { a.ln_ld = T; a.ln_D = K; a.ln_eps = 1e-5f; }
  }
  return a;
}

// MXFP8 decoration of a built block Linear (an MXFP8 net, Mode::f8).  A8: the MXFP8 A operand in place of the bf16
// one, on the block-scaled MFMA against the e4m3 weight + its "_scale"; a LayerNorm consumer then takes A
// group-centred (GemmArgs::ln_gcol).  A8 null: a bf16 Linear (skip_linear, a bf16 fc1).  out8.q set: the epilogue
// also writes the MXFP8 copy of what it stores, the next Linear's operand, group-centred when written beside
// LayerNorm partials (GemmArgs::mx_center).
void mx_decorate(const pdm_uvit* h, pdm::GemmArgs& a, const Q8* A8, const LinW& lw, const Q8& out8) {
  if (A8) {
    a.A1 = (const bf16*)A8->q; a.lda1 = A8->ld;
    a.fp8 = 1;
    a.a_scale = A8->s; a.a_scale_ld = A8->sld;
    a.w_scale = lw.scale; a.w_scale_ld = a.N;
    if (a.ln_stats) a.ln_gcol = lw.gcol;
    a.ln_ld = (h->D + 255) / 256; a.ln_D = a.K; a.ln_eps = 1e-5f;
  }
  a.out_fp8 = out8.q; a.ldo8 = out8.ld; a.out_scale = out8.s; a.out_scale_ld = out8.sld;
  a.mx_center = out8.q && a.stats_out ? 1 : 0;
  // an MXFP8 net's launches have always carried the leading dimensions of their present outputs only
  a.ldo = a.out_bf16 ? a.N : 0;
  a.ldr = a.out_f32 ? h->D : 0;
  a.ldri = a.res_in ? a.N : 0;
}

// One stream of a block: weights, rows, where x comes from and goes to, and the block's scratch
struct BlockIO {
  const BlockW* W;
  int L;                 // tokens per sequence
  float* X;              // fp32 stream: the residual rows [rows L, D], updated in place; null on the bf16 stream
  const bf16* xin;       // the block input: x itself (bf16 stream) or its bf16 copy (fp32 stream)
  const float* st_in;    // LayerNorm partials of the input
  const bf16* skip_in;   // long-skip activation [rows L, D] (out-blocks), or null
  bf16* xout;            // where fc2 leaves the block output in bf16 (fp32 stream: may be null)
  float* st_out;         // and its partials (fp32 stream: may be null)
  bf16 *XT, *QKV, *ATT, *MLP;   // scratch: the block-internal x (bf16), qkv, attention output, GELU(fc1)
  float* STT;                   // partials of the block-internal x
  Q8 in8, out8;          // MXFP8 net: the input as the qkv operand; where fc2 leaves the output for the next qkv
};

// One U-ViT Block (libs/uvit.py:115-120) for n = 1 or 2 streams in lockstep, norm1 / norm2 fused into qkv / fc1:
//   [x = skip_linear(cat([x, skip]))]  qkv = norm1(x) W^T  attention  x += proj(attn)  h = GELU(fc1(norm2(x)))
//   x += fc2(h)
// Each producing epilogue (skip_linear, proj, fc2) leaves x and its LayerNorm partials in the form its consumer
// reads.  Two streams (the mask and the image block of a t2i layer: same D / Hid, different weights, rows and
// buffers) share every Linear as one grouped launch; attention runs per stream.  In an MXFP8 net (one stream) the
// Linears' operands are the workspace's MXFP8 buffers: xtq the block-internal x, atq the attention output, mlq
// GELU(fc1), which is then stored only so.  skip_linear stays bf16 there: its output REPLACES the residual stream,
// and in MXFP8 it alone costs 6.3e-2 rel-L2 of the H/4 forward for 7 % of the FLOPs; attention stays
// bf16 too (a 72-deep QK^T cannot fill the 128-deep scaled MFMA).
int run_block(const Ctx& c, Mode m, int nseq, int n, const BlockIO* io, const Workspace& w) {
  const pdm_uvit* h = c.h;
  const int D = h->D, Hid = h->Hid;
  const bool f8 = m.f8 != 0, fc1_8 = (m.f8 & 4) != 0;
  const int res_epi = m.r16 ? pdm::EPI_RES : pdm::EPI_F32;
  if (n == 2 && (f8 || !io[0].skip_in != !io[1].skip_in))
    return fail(PDM_ERR_STATE, "run_block: paired streams are bf16 Linears with long skips in both or neither");
  pdm::GemmArgs g[2];
  auto launch = [&](int epi) { return n == 2 ? launch_gemm_pair(c, g[0], g[1], epi) : launch_gemm(c, g[0], epi); };
  // XT as the bf16 operand of block Linear `bit`: the bf16 stream's x is there anyway; the fp32 stream stores the
  // copy only for a bf16 consumer
  auto xt = [&](const BlockIO& s, int bit) { return m.r16 || !((m.f8 >> bit) & 1) ? s.XT : nullptr; };
  const bf16* x[2] = {io[0].xin, n == 2 ? io[1].xin : nullptr};
  const float* st[2] = {io[0].st_in, n == 2 ? io[1].st_in : nullptr};
  Q8 x8 = io[0].in8;
  if (io[0].skip_in) {  // x = skip_linear(cat([x, skip], -1)): split-K over the two bf16 operands
    for (int i = 0; i < n; ++i) {
      const BlockIO& s = io[i];
      g[i] = res_lin(h, m, s.xin, D, s.skip_in, s.W->skip, nseq * s.L, 2 * D, s.X, nullptr, xt(s, 0), s.STT);
      if (f8) mx_decorate(h, g[i], nullptr, s.W->skip, w.xtq);
      x[i] = s.XT;
      st[i] = s.STT;
    }
    PDM_TRY(launch(res_epi));
    x8 = w.xtq;
  }
  for (int i = 0; i < n; ++i) {  // qkv = norm1(x) W^T (bf16 for the attention kernel)
    const BlockIO& s = io[i];
    g[i] = ln_lin(h, x[i], s.W->qkv, nseq * s.L, 3 * D, D, s.QKV, st[i]);
    if (f8) mx_decorate(h, g[i], &x8, s.W->qkv, Q8());
  }
  PDM_TRY(launch(pdm::EPI_BF16));
  for (int i = 0; i < n; ++i) {
    const BlockIO& s = io[i];
    pdm::AttentionArgs a{};
    a.qkv = s.QKV; a.ldq = 3 * D;
    a.out = s.ATT; a.ldo = D;
    a.B = nseq; a.L = s.L; a.H = h->H; a.Dh = h->Dh;
    a.scale = 1.0f / sqrtf((float)h->Dh);
    a.q_log2 = 1;   // attn.qkv's q rows are packed pre-scaled by Dh^-0.5 log2(e) (include/pdm.h)
    PDM_CHECK(pdm::attention_check(a));
    PDM_HIP(pdm::attention_launch(a, c.s));
    if (f8) PDM_HIP(pdm::mxq_launch(s.ATT, 1, D, nseq * s.L, D, w.atq.q, w.atq.ld, w.atq.s, w.atq.sld, c.s));
  }
  for (int i = 0; i < n; ++i) {  // x += proj(attn) -> X / XT (xin itself may be a long-skip operand kept for later)
    const BlockIO& s = io[i];
    g[i] = res_lin(h, m, s.ATT, D, nullptr, s.W->proj, nseq * s.L, D, s.X, x[i], xt(s, 2), s.STT);
    if (f8) mx_decorate(h, g[i], &w.atq, s.W->proj, fc1_8 ? w.xtq : Q8());
  }
  PDM_TRY(launch(res_epi));
  for (int i = 0; i < n; ++i) {  // h = GELU(fc1(norm2(x)))
    const BlockIO& s = io[i];
    g[i] = ln_lin(h, s.XT, s.W->fc1, nseq * s.L, Hid, D, f8 ? nullptr : s.MLP, s.STT);
    if (f8) mx_decorate(h, g[i], fc1_8 ? &w.xtq : nullptr, s.W->fc1, w.mlq);
    if (f8 && !fc1_8) g[i].stats_ld = 0;   // (the bf16 fc1 of an MXFP8 net has always carried 0 here)
  }
  PDM_TRY(launch(pdm::EPI_GELU));
  for (int i = 0; i < n; ++i) {  // x += fc2(h) -> X / xout
    const BlockIO& s = io[i];
    g[i] = res_lin(h, m, s.MLP, Hid, nullptr, s.W->fc2, nseq * s.L, Hid, s.X, s.XT, s.xout, s.st_out);
    if (f8) mx_decorate(h, g[i], &w.mlq, s.W->fc2, s.out8);
  }
  return launch(res_epi);
}

// a block stream on the workspace's first scratch set
BlockIO block_io(const Workspace& w, const BlockW& W, int L) {
  BlockIO s{};
  s.W = &W; s.L = L;
  s.XT = w.XT; s.QKV = w.QKV; s.ATT = w.ATT; s.MLP = w.MLP; s.STT = w.STT;
  return s;
}

// bf16 copy + LayerNorm partials of fp32 rows no GEMM epilogue produced (token assembly, mask-stream refresh)
int row_stats(const Ctx& c, const float* X, int rows, bf16* xb, float* st) {
  const int D = c.h->D;
  PDM_HIP(pdm::rowstats_launch(X, D, rows, D, xb, D, st, (D + 255) / 256, c.s));
  return PDM_OK;
}

// The single-stream block stack (libs/uvit.py:213-222, libs/uvit_t2i.py:407-410 / 516) over the assembled fp32
// tokens X.  Every activation is produced once, by the epilogue that computes it, in the precision and layout of
// its consumers; what a block leaves for the next one, in every mode:
//   * the LayerNorm partials of its output, in ST;
//   * its output in bf16 -- x itself on the bf16 stream, else the copy a bf16 qkv, a skip_linear or a long skip
//     reads: an in-block's in SK[i], the long-skip slot (with bf16 Linears always: it is also the next block's
//     operand; in an MXFP8 net only if the net has long skips), every other block's in XB.  The fp32 stream of an
//     MXFP8 net without long skips has no bf16 reader, and none is stored;
//   * in an MXFP8 net also its output as MXFP8 in xq, the next qkv operand, unless the next block starts with
//     skip_linear (bf16 operands).
// A block reads its input before its fc2 writes the output, so XB is updated in place.  The last out-block of the
// fp32 stream leaves nothing but X (the final norm reads it); on the bf16 stream XB is the result.
int run_stack(const Ctx& c, Mode m, const Workspace& w, int rows, int L) {
  const pdm_uvit* h = c.h;
  const int D = h->D, M = rows * L;
  const size_t MD = (size_t)M * D;
  const bool f8 = m.f8 != 0, skip = h->cfg.skip != 0;
  const bool no_bf16 = f8 && !m.r16 && !skip;
  bf16* xb0 = f8 && !m.r16 ? nullptr : w.XB;   // (MXFP8 net, fp32 stream: the first qkv reads xq)
  PDM_HIP(pdm::rowstats_launch(w.X, D, M, D, xb0, xb0 ? D : 0, w.ST, (D + 255) / 256, c.s, w.xq.q, w.xq.ld, w.xq.s,
                               w.xq.sld, f8 ? 1 : 0));
  const bf16* x = w.XB;
  for (const Layer& ly : h->layers) {
    const bool last = ly.last && !m.r16;
    BlockIO s = block_io(w, ly.img, L);
    s.X = m.r16 ? nullptr : w.X;
    s.xin = x; s.st_in = w.ST;
    s.skip_in = ly.skip_from >= 0 ? w.SK + ly.skip_from * MD : nullptr;
    s.xout = ly.keep >= 0 && (skip || !f8) ? w.SK + ly.keep * MD : last || no_bf16 ? nullptr : w.XB;
    s.st_out = last ? nullptr : w.ST;
    s.in8 = w.xq;
    if (f8 && !last && (ly.keep >= 0 || !skip)) s.out8 = w.xq;
    PDM_TRY(run_block(c, m, rows, 1, &s, w));
    x = s.xout;
  }
  return PDM_OK;
}

// every weight registered; the resolved table follows the registrations (pdm_uvit_set_param marks it dirty)
int check_ready(pdm_uvit* h) {
  if (!h->dirty) return PDM_OK;
  for (auto& n : h->order)
    if (!h->params[n].ptr) return fail(PDM_ERR_STATE, "pdm_uvit: weight not registered: " + n);
  h->resolve();
  return PDM_OK;
}

// What both forward entry points do before the first launch: the weights resolved, the workspace laid out and
// checked, the profiling hook rewound, the forward's stream-K state
int begin_forward(pdm_uvit* h, const char* who, int rows, void* workspace, size_t workspace_bytes, void* stream,
                  Workspace& w, Ctx& c) {
  PDM_TRY(check_ready(h));
  w = layout(h, rows, (char*)workspace);
  if (w.bytes > workspace_bytes) return fail(PDM_ERR_ARG, std::string(who) + ": workspace too small");
  h->prof_n = 0;
  c.h = h;
  c.s = (hipStream_t)stream;
  return sk_begin(c, &c.sk_used);
}

// The image stream's tokens [label?, time, context x n_ctx?, patches] + pos_embed -> the first Lx rows of each
// L_total-row sequence of X (libs/uvit.py:205-211: [label, time, patches]; libs/uvit_t2i.py:401-405 / 408-409:
// [time, context, patches]); only pos_embed rows [0, Lx) are read
int assemble_image(const Ctx& c, const Workspace& w, const float* x, const float* t, const int64_t* y, int rows,
                   int L_total) {
  const pdm_uvit* h = c.h;
  const bool t2i = h->cfg.t2i != 0;
  pdm::AssembleArgs a{};
  a.img = x; a.C = h->C; a.Himg = h->cfg.img_size; a.Wimg = h->cfg.img_size; a.p = h->p;
  a.patch_w = h->patch_w; a.patch_b = h->patch_b;
  a.t = t; a.y = y;
  a.label_emb = h->label_emb;
  if (t2i) { a.ctx_tokens = w.CTXF; a.n_ctx = h->cfg.num_clip_token; }
  a.pos = h->pos;
  a.out = w.X; a.ld_out = h->D;
  a.B = rows; a.D = h->D; a.L_total = L_total;
  a.row0_patch = h->extras;
  a.time_row = t2i ? 0 : h->extras - 1;
  a.label_row = y ? 0 : -1;
  a.ctx_row = t2i ? 1 : -1;
  PDM_CHECK(pdm::assemble_check(a));
  PDM_HIP(pdm::assemble_launch(a, c.s));
  return PDM_OK;
}

// The mask patches mask_embed(mask_token) + pos -> rows [Lx, Lm) of each Lm-row sequence that starts at `out`
int assemble_mask(const Ctx& c, const float* mask_token, const float* pos, float* out, int rows) {
  const pdm_uvit* h = c.h;
  pdm::AssembleArgs a{};
  a.img = mask_token; a.C = h->K; a.Himg = h->cfg.img_size; a.Wimg = h->cfg.img_size; a.p = h->p;
  a.patch_w = h->mask_w; a.patch_b = h->mask_b;
  a.pos = pos;
  a.out = out + (size_t)h->Lx * h->D; a.ld_out = h->D; a.B = rows; a.D = h->D; a.L_total = h->Lm;
  a.row0_patch = 0; a.time_row = -1; a.label_row = -1; a.ctx_row = -1;
  PDM_CHECK(pdm::assemble_check(a));
  PDM_HIP(pdm::assemble_launch(a, c.s));
  return PDM_OK;
}

// decoder_pred-style head on bf16 token rows: token (b, i) is row b * group_stride + row_offset + i of `hin`.
int run_head(const Ctx& c, const bf16* hin, int group_stride, int row_offset, int rows, const LinW& head, int Cout,
             int P, int P_pad, float* out) {
  const pdm_uvit* h = c.h;
  pdm::HeadArgs a{};
  a.x = hin; a.ldx = h->D;
  a.in_group_stride = group_stride; a.in_row_offset = row_offset;
  a.W = head.w; a.bias = head.bias;
  a.out = out;
  a.B = rows; a.D = h->D; a.C = Cout; a.p = h->p; a.Himg = h->cfg.img_size; a.Wimg = h->cfg.img_size;
  a.P = P; a.P_pad = P_pad; a.act_tanh = 0;
  PDM_CHECK(pdm::head_check(a));
  PDM_HIP(pdm::head_launch(a, c.s));
  return PDM_OK;
}

// The final LayerNorm over rows [extras, extras + per_seq) of each L-row sequence of the result (XB on the bf16
// stream, X on the fp32 one) -> HEADIN [rows][per_seq][D]; a caller adds what its tail sums into the norm
pdm::LayerNormArgs final_norm(const pdm_uvit* h, const Workspace& w, int rows, int L, int per_seq) {
  pdm::LayerNormArgs a{};
  if (h->res16()) a.xb = w.XB; else a.x = w.X;
  a.ldx = h->D;
  a.gamma = h->norm_w; a.beta = h->norm_b;
  a.y = w.HEADIN; a.ldy = h->D;
  a.rows = rows * per_seq; a.D = h->D;
  a.rows_per_group = per_seq; a.group_stride = L; a.row_offset = h->extras;
  a.eps = 1e-5f;
  a.add_ld = h->D;
  return a;
}

// The tail of every forward: the final norm, the mask head on rows (group stride mask_gs, offset mask_off) of
// mask_in unless that is null, then the noise head on the first n_patch rows of each HEADIN group
int run_tail(const Ctx& c, const Workspace& w, int rows, const pdm::LayerNormArgs& ln, const bf16* mask_in,
             int mask_gs, int mask_off, float* eps_pre, float* mask_pre) {
  const pdm_uvit* h = c.h;
  PDM_CHECK(pdm::layernorm_check(ln));
  PDM_HIP(pdm::layernorm_launch(ln, c.s));
  if (mask_in) PDM_TRY(run_head(c, mask_in, mask_gs, mask_off, rows, h->head_mask, h->K, h->PK, h->PK_pad, mask_pre));
  return run_head(c, w.HEADIN, ln.rows_per_group, 0, rows, h->head, h->C, h->P, h->P_pad, eps_pre);
}

// The panoptic two-stream U-ViT (libs/uvit_t2i.py:411-525) on the bf16 residual stream, after the image tokens
// (X) and the mask tokens (MX[:, Lx:]) were assembled in fp32.  Per layer: the mask stream input mb = cat(x, m)
// is rebuilt in MB (image rows copied from the image block's INPUT x, 426 / 443 / 459; mask rows from the
// previous mask block's output), both blocks run, then x += zeroconv(mask block output[:, :Lx]) (435-436,
// 452-453, 470-472) as a residual GEMM into the image output buffer.
int t2i_two_stream16(const Ctx& c, Mode m, const Workspace& w, int rows, int use_ground_truth, float* eps_pre,
                     float* mask_pre) {
  const pdm_uvit* h = c.h;
  const int D = h->D, Lx = h->Lx, Lm = h->Lm, T = (D + 255) / 256;
  const size_t MDx = (size_t)rows * Lx * D, MDm = (size_t)rows * Lm * D;
  // the image block's own scratch: always present here, since layout() allocates it for every separate panoptic net
  // on the bf16 stream without MXFP8, and pdm_uvit_create rejects MXFP8 t2i nets
  if (!w.XT2) return fail(PDM_ERR_STATE, "t2i_two_stream16: no image-stream scratch in this workspace");
  // bf16 row copies of D columns (as fp32 words: D / 2 per row), optionally with the rows' LayerNorm partials
  auto copy_rows = [&](bf16* dst, const bf16* src, int rpg, int dgs, int sgs, float* st_dst = nullptr,
                       const float* st_src = nullptr) -> int {
    PDM_HIP(pdm::rowcopy_launch((float*)dst, D / 2, (const float*)src, D / 2, rows * rpg, D / 2, rpg, dgs, sgs, c.s,
                                st_dst, 2 * T, st_src, 2 * T, 2 * T));
    return PDM_OK;
  };
  // image tokens -> XB + ST; mask tokens -> MB[:, Lx:] (the image rows of this pass are overwritten by the refresh)
  PDM_TRY(row_stats(c, w.X, rows * Lx, w.XB, w.ST));
  PDM_TRY(row_stats(c, w.MX, rows * Lm, w.MB, w.STM));
  const bf16* x = w.XB;
  const bf16* mprev = w.MB;
  for (const Layer& ly : h->layers) {
    // refresh mb = cat(x, m) + its partials.  The image rows and their partials came from the previous layer's
    // injection (its second output), and only before the first layer from x itself (XB / ST of the assembly).  The
    // mask rows' partials are already in STM, written by the mask block that produced them (its fc2 epilogue) or by
    // the token assembly; the rows themselves are copied unless already in place.
    if (&ly == &h->layers.front()) PDM_TRY(copy_rows(w.MB, x, Lx, Lm, Lx, w.STM, w.ST));
    if (mprev != w.MB) PDM_TRY(copy_rows(w.MB + (size_t)Lx * D, mprev + (size_t)Lx * D, Lm - Lx, Lm, Lm));
    // the mask block and the image block in lockstep, every Linear of the pair one grouped launch.  The mask block
    // only needs the image block's INPUT x; the image block's output stays in its scratch XT2 (proj / fc2 update it
    // in place), and its fc2 partials, which nobody reads (the injection produces x's), land in STT2 so that both
    // fc2s take the same epilogue and group.
    bf16* mout = ly.keep >= 0 ? w.SKM + ly.keep * MDm : w.MXB;
    bf16* xout = ly.keep >= 0 ? w.SK + ly.keep * MDx : w.XB;
    BlockIO io[2] = {block_io(w, ly.mask, Lm), block_io(w, ly.img, Lx)};
    io[0].xin = w.MB; io[0].st_in = w.STM; io[0].xout = mout; io[0].st_out = w.STM;
    io[1].xin = x; io[1].st_in = w.ST; io[1].xout = w.XT2; io[1].st_out = w.STT2;
    io[1].XT = w.XT2; io[1].QKV = w.QKV2; io[1].ATT = w.ATT2; io[1].MLP = w.MLP2; io[1].STT = w.STT2;
    if (ly.skip_from >= 0) {
      io[0].skip_in = w.SKM + ly.skip_from * MDm;
      io[1].skip_in = w.SK + ly.skip_from * MDx;
    }
    PDM_TRY(run_block(c, m, rows, 2, io, w));
    // inject: x_out = x + zeroconv(mout[:, :Lx]), also stored (with its partials) as the image rows of MB -- the
    // next layer's mask-stream input; mout (SKM[i] / MXB) is never MB, so no tile reads rows another one writes
    pdm::GemmArgs a = res_lin(h, m, mout, D, nullptr, ly.zc, rows * Lx, D, nullptr, w.XT2, xout, w.ST);
    a.a_rows_per_group = Lx; a.a_group_stride = Lm;
    a.out2 = w.MB; a.out2_rpg = Lx; a.out2_gs = Lm;
    a.stats_out2 = w.STM;
    PDM_TRY(launch_gemm(c, a, pdm::EPI_RES));
    x = xout;
    mprev = mout;
  }
  // heads (477-519): noise from norm(x) patch tokens (+ the mask rows, use_ground_truth: 486-494); the mask head on
  // the un-normalised m (the last mask output)
  pdm::LayerNormArgs ln = final_norm(h, w, rows, Lx, h->n_patch);
  if (use_ground_truth) { ln.addb = w.MXB; ln.add_group_stride = Lm; ln.add_row_offset = Lx; }
  return run_tail(c, w, rows, ln, use_ground_truth ? nullptr : w.MXB, Lm, Lx, eps_pre, mask_pre);
}

// The same network on the fp32 residual stream: x in X, the mask stream mx = cat(x, m) in MX, one block after the
// other.  Before every mask block the image half of MX is refreshed from X (426, 443, 459) and the whole mask
// stream's bf16 copy + partials redone (its blocks' qkv / skip_linear operand); the injection adds into X and
// leaves bf16 of the new x (the long skip / next block's operand) and its partials.
int t2i_two_stream32(const Ctx& c, Mode m, const Workspace& w, int rows, int use_ground_truth, float* eps_pre,
                     float* mask_pre) {
  const pdm_uvit* h = c.h;
  const int D = h->D, Lx = h->Lx, Lm = h->Lm;
  const size_t MDx = (size_t)rows * Lx * D, MDm = (size_t)rows * Lm * D;
  PDM_TRY(row_stats(c, w.X, rows * Lx, w.XB, w.ST));
  const bf16* xb = w.XB;
  for (const Layer& ly : h->layers) {
    PDM_HIP(pdm::rowcopy_launch(w.MX, D, w.X, D, rows * Lx, D, Lx, Lm, Lx, c.s));
    PDM_TRY(row_stats(c, w.MX, rows * Lm, w.MXIN, w.STM));
    bf16* mout = ly.keep >= 0 ? w.SKM + ly.keep * MDm : w.MXB;
    bf16* xout = ly.keep >= 0 ? w.SK + ly.keep * MDx : w.XB;
    BlockIO si = block_io(w, ly.img, Lx), sm = block_io(w, ly.mask, Lm);
    si.X = w.X; si.xin = xb; si.st_in = w.ST;
    sm.X = w.MX; sm.xin = w.MXIN; sm.st_in = w.STM; sm.xout = mout;
    if (ly.skip_from >= 0) {
      si.skip_in = w.SK + ly.skip_from * MDx;
      sm.skip_in = w.SKM + ly.skip_from * MDm;
    }
    PDM_TRY(run_block(c, m, rows, 1, &si, w));
    PDM_TRY(run_block(c, m, rows, 1, &sm, w));
    // inject: x += zeroconv(mx[:, :Lx]) from the bf16 copy of the mask block output
    pdm::GemmArgs a = res_lin(h, m, mout, D, nullptr, ly.zc, rows * Lx, D, w.X, nullptr, xout, w.ST);
    a.a_rows_per_group = Lx; a.a_group_stride = Lm;
    PDM_TRY(launch_gemm(c, a, pdm::EPI_F32));
    xb = xout;
  }
  // heads: as on the bf16 stream, with the un-normalised m = MX[:, Lx:] in fp32 and its bf16 copy MXB
  pdm::LayerNormArgs ln = final_norm(h, w, rows, Lx, h->n_patch);
  if (use_ground_truth) { ln.add = w.MX; ln.add_group_stride = Lm; ln.add_row_offset = Lx; }
  return run_tail(c, w, rows, ln, use_ground_truth ? nullptr : w.MXB, Lm, Lx, eps_pre, mask_pre);
}

}  // namespace

// ==================================================================================================
extern "C" {

const char* pdm_last_error(void) { return g_err.c_str(); }

int pdm_version(void) { return 1; }

int pdm_set_gemm_algo(int algo) {
  if (algo < 0 || algo > 11 || algo == 10)
    return fail(PDM_ERR_ARG, "pdm_set_gemm_algo: algo must be 0 (auto), 1..9 or 11");
  pdm::gemm_set_algo(algo);
  return PDM_OK;
}

int pdm_set_gemm_sk(int mode) {
  if ((mode & 3) > 2 || mode < 0 || mode > 7) return fail(PDM_ERR_ARG, "pdm_set_gemm_sk: mode must be 0..2 (+4)");
  pdm::gemm_set_sk(mode & 3);
  g_sk_standalone = (mode & 4) != 0;
  return PDM_OK;
}

long long pdm_gemm_sk_launches(void) { return pdm::gemm_sk_launches(); }

int pdm_gemm_seg_stats(unsigned long long* out25) {
  if (!out25) return fail(PDM_ERR_ARG, "pdm_gemm_seg_stats: null output");
  if (pdm::gemm_seg_stats(out25)) return fail(PDM_ERR_HIP, "pdm_gemm_seg_stats: device copy failed");
  return PDM_OK;
}
int pdm_gemm_sk_stats(unsigned long long* out3) {
  if (!out3) return fail(PDM_ERR_ARG, "pdm_gemm_sk_stats: null output");
  if (pdm::gemm_sk_stats(out3)) return fail(PDM_ERR_HIP, "pdm_gemm_sk_stats: device copy failed");
  return PDM_OK;
}

int pdm_set_gemm_tuning(int raster, int dbg_tile0) {
  if (raster < 0 || raster > 64) return fail(PDM_ERR_ARG, "pdm_set_gemm_tuning: raster must be in [0, 64]");
  pdm::gemm_set_tuning(raster, dbg_tile0);
  return PDM_OK;
}

int pdm_set_attention_algo(int algo) {
  if (algo < 0 || algo > 16)
    return fail(PDM_ERR_ARG, "pdm_set_attention_algo: algo must be 0 (auto) or 1..16 (5, 6, 8, 9, 12, 13, 15, 16: timing "
                             "experiments)");
  pdm::attention_set_algo(algo);
  return PDM_OK;
}

int pdm_attention_plan(int B, int L, int H, int Dh, int algo, int ncu, int* out6) {
  if (!out6) return fail(PDM_ERR_ARG, "pdm_attention_plan: null output");
  if (algo < 0 || algo > 16) return fail(PDM_ERR_ARG, "pdm_attention_plan: algo must be in [0, 16]");
  if (ncu < 0) return fail(PDM_ERR_ARG, "pdm_attention_plan: ncu must be >= 0 (0: the default, 256)");
  pdm::AttentionArgs a{};   // the shape checks of pdm_attention on dense, aligned (never dereferenced) operands
  a.ldq = 3 * H * Dh; a.ldo = H * Dh; a.B = B; a.L = L; a.H = H; a.Dh = Dh;
  PDM_CHECK(pdm::attention_check(a));
  const pdm::AttentionPlan pl = pdm::attention_plan(B, L, H, Dh, algo, ncu ? ncu : 256);
  out6[0] = pl.family; out6[1] = pl.waves; out6[2] = pl.tail1; out6[3] = pl.variant; out6[4] = pl.grid;
  out6[5] = pl.lds_bytes;
  return PDM_OK;
}

int pdm_device_arch(char* buf, int len) {
  int dev = 0;
  PDM_HIP(hipGetDevice(&dev));
  hipDeviceProp_t prop;
  PDM_HIP(hipGetDeviceProperties(&prop, dev));
  snprintf(buf, len, "%s", prop.gcnArchName);
  return PDM_OK;
}

int pdm_uvit_create(const pdm_uvit_cfg* cfg, pdm_uvit** out) {
  if (!cfg || !out) return fail(PDM_ERR_ARG, "pdm_uvit_create: null argument");
  const pdm_uvit_cfg& c = *cfg;
  if (c.embed_dim <= 0 || c.num_heads <= 0 || c.embed_dim % c.num_heads) return fail(PDM_ERR_ARG, "embed_dim must be divisible by num_heads");
  if (c.patch_size <= 0 || c.img_size % c.patch_size) return fail(PDM_ERR_ARG, "img_size must be divisible by patch_size");
  if (c.mlp_time_embed) return fail(PDM_ERR_ARG, "mlp_time_embed=True is not supported by the HIP path");
  if (c.embed_dim % 64) return fail(PDM_ERR_ARG, "embed_dim must be a multiple of 64");
  if (c.mlp_hidden % 64) return fail(PDM_ERR_ARG, "mlp hidden size must be a multiple of 64");
  if (c.fp8 && c.t2i) return fail(PDM_ERR_ARG, "fp8: only the class-conditional / unconditional U-ViT has an MXFP8 path");
  if (c.fp8 && (c.embed_dim % 128 || c.mlp_hidden % 128))
    return fail(PDM_ERR_ARG, "fp8: embed_dim and the mlp hidden size must be multiples of 128 (MXFP8 K-tiles)");
  if (c.fp8 && c.fp8_linears != 0 && c.fp8_linears != 0xF && c.fp8_linears != 0xB)
    return fail(PDM_ERR_ARG, "fp8_linears: supported sets are all four block Linears (0 / 0xF) and 0xB (mlp.fc1 bf16)");
  if (c.embed_dim > 2048 && c.fp8) return fail(PDM_ERR_ARG, "fp8: embed_dim must be <= 2048 (centred LayerNorm groups)");
  pdm_uvit* h = new pdm_uvit();
  h->cfg = c;
  h->D = c.embed_dim;
  h->H = c.num_heads;
  h->Dh = c.embed_dim / c.num_heads;
  h->Hid = c.mlp_hidden;
  h->C = c.in_chans;
  h->p = c.patch_size;
  h->n_patch = (c.img_size / c.patch_size) * (c.img_size / c.patch_size);
  h->depth = c.depth;
  h->nhalf = c.depth / 2;
  h->P = c.patch_size * c.patch_size * c.in_chans;
  h->P_pad = (h->P + 15) / 16 * 16;
  h->K = c.num_panoptic_class;
  h->PK = c.patch_size * c.patch_size * c.num_panoptic_class;
  h->PK_pad = (h->PK + 15) / 16 * 16;
  if (h->P_pad > 64 || (c.t2i && c.enable_panoptic && h->PK_pad > 64)) {
    delete h;
    return fail(PDM_ERR_ARG, "patch_size^2 * channels must be <= 64");
  }
  if (!c.t2i) {
    h->extras = c.num_classes > 0 ? 2 : 1;
  } else {
    h->extras = 1 + c.num_clip_token;
    if (c.clip_dim % 64) {
      delete h;
      return fail(PDM_ERR_ARG, "clip_dim must be a multiple of 64");
    }
  }
  h->Lx = h->extras + h->n_patch;
  h->Lm = h->Lx + h->n_patch;
  const int D = h->D;
  const int pk = c.in_chans * c.patch_size * c.patch_size;
  h->add("pos_embed", PDM_F32, (long long)(h->joint() ? h->Lm : h->Lx) * D);   // joint: rows [Lx, Lm) = mask patches
  h->add("patch_embed.proj.weight", PDM_F32, (long long)D * pk);
  h->add("patch_embed.proj.bias", PDM_F32, D);
  if (!c.t2i && c.num_classes > 0) h->add("label_emb.weight", PDM_F32, (long long)c.num_classes * D);
  if (c.t2i) {
    h->add("context_embed.weight", PDM_BF16, (long long)D * c.clip_dim);
    h->add("context_embed.bias", PDM_F32, D);
  }
  h->add_stack("");
  h->add("norm.weight", PDM_F32, D);
  h->add("norm.bias", PDM_F32, D);
  h->add("decoder_pred.weight", PDM_BF16, (long long)h->P_pad * D);
  h->add("decoder_pred.bias", PDM_F32, h->P);
  if (c.t2i && c.enable_panoptic && c.separate) {
    h->add("pos_embed_mask", PDM_F32, (long long)h->n_patch * D);
    h->add("mask_embed.proj.weight", PDM_F32, (long long)D * h->PK);
    h->add("mask_embed.proj.bias", PDM_F32, D);
    h->add("decoder_pred_mask.weight", PDM_BF16, (long long)h->PK_pad * D);
    h->add("decoder_pred_mask.bias", PDM_F32, h->PK);
    h->add_stack("_mask");
    for (int i = 0; i <= c.depth; ++i) {
      h->add(pdm_uvit::zc_name(i) + ".weight", PDM_BF16, (long long)D * D);
      h->add(pdm_uvit::zc_name(i) + ".bias", PDM_F32, D);
    }
  }
  if (h->joint()) {   // one stack: the mask patches' embedding and head only (mask_embed_0 is unused: 392-396)
    h->add("mask_embed.proj.weight", PDM_F32, (long long)D * h->PK);
    h->add("mask_embed.proj.bias", PDM_F32, D);
    h->add("decoder_pred_mask.weight", PDM_BF16, (long long)h->PK_pad * D);
    h->add("decoder_pred_mask.bias", PDM_F32, h->PK);
  }
  const int n = h->nhalf;
  h->layers.resize(2 * n + 1);
  for (int l = 0; l <= 2 * n; ++l) {
    Layer& ly = h->layers[l];
    if (l < n) ly.keep = l;
    if (l > n && c.skip) ly.skip_from = 2 * n - l;   // out-block i reads in-block n - 1 - i (libs/uvit.py:219-220)
    ly.last = n > 0 && l == 2 * n;
  }
  *out = h;
  return PDM_OK;
}

int pdm_uvit_destroy(pdm_uvit* h) {
  if (h)
    for (auto e : h->prof_ev) (void)hipEventDestroy(e);
  delete h;
  return PDM_OK;
}

int pdm_uvit_profile(pdm_uvit* h, int max_launches) {
  if (!h || max_launches < 0) return fail(PDM_ERR_ARG, "pdm_uvit_profile: bad argument");
  if (max_launches == 0) {
    h->prof_on = false;
    return PDM_OK;
  }
  while ((int)h->prof_ev.size() < 2 * max_launches) {
    hipEvent_t e;
    PDM_HIP(hipEventCreate(&e));
    h->prof_ev.push_back(e);
  }
  h->prof_flops.assign(max_launches, 0.0);
  h->prof_n = 0;
  h->prof_on = true;
  return PDM_OK;
}

int pdm_uvit_profile_read(pdm_uvit* h, float* ms, double* flops, int cap, int* n) {
  if (!h || !n) return fail(PDM_ERR_ARG, "pdm_uvit_profile_read: bad argument");
  *n = h->prof_n;
  for (int i = 0; i < h->prof_n && i < cap; ++i) {
    PDM_HIP(hipEventSynchronize(h->prof_ev[2 * i + 1]));
    PDM_HIP(hipEventElapsedTime(&ms[i], h->prof_ev[2 * i], h->prof_ev[2 * i + 1]));
    flops[i] = h->prof_flops[i];
  }
  return PDM_OK;
}

int pdm_uvit_param_count(const pdm_uvit* h) { return h ? (int)h->order.size() : 0; }

int pdm_uvit_param_info(const pdm_uvit* h, int i, char* name, int len, int* dtype, long long* numel) {
  if (!h || i < 0 || i >= (int)h->order.size()) return fail(PDM_ERR_ARG, "pdm_uvit_param_info: index out of range");
  const std::string& n = h->order[i];
  snprintf(name, len, "%s", n.c_str());
  const ParamSpec& s = h->params.at(n);
  *dtype = s.dtype;
  *numel = s.numel;
  return PDM_OK;
}

int pdm_uvit_set_param(pdm_uvit* h, const char* name, const void* dev_ptr, int dtype, long long numel) {
  if (!h || !name) return fail(PDM_ERR_ARG, "pdm_uvit_set_param: null argument");
  auto it = h->params.find(name);
  if (it == h->params.end()) return fail(PDM_ERR_ARG, std::string("pdm_uvit_set_param: unexpected key ") + name);
  if (it->second.dtype != dtype || it->second.numel != numel)
    return fail(PDM_ERR_ARG, std::string("pdm_uvit_set_param: dtype/size mismatch for ") + name);
  if (((uintptr_t)dev_ptr) & 15) return fail(PDM_ERR_ARG, std::string("pdm_uvit_set_param: 16-byte alignment required for ") + name);
  it->second.ptr = dev_ptr;
  h->dirty = true;
  return PDM_OK;
}

int pdm_uvit_validate(pdm_uvit* h) {
  if (!h) return fail(PDM_ERR_ARG, "null handle");
  return check_ready(h);
}

int pdm_uvit_workspace_size(const pdm_uvit* h, int rows, size_t* bytes) {
  if (!h || rows <= 0 || !bytes) return fail(PDM_ERR_ARG, "pdm_uvit_workspace_size: bad argument");
  *bytes = layout(h, rows, nullptr).bytes;
  return PDM_OK;
}

int pdm_uvit_forward(pdm_uvit* h, const float* x, const float* t, const int64_t* y, float* eps_pre, int rows,
                     void* workspace, size_t workspace_bytes, void* stream) {
  if (!h || !x || !t || !eps_pre || rows <= 0) return fail(PDM_ERR_ARG, "pdm_uvit_forward: bad argument");
  if (h->cfg.t2i) return fail(PDM_ERR_ARG, "pdm_uvit_forward: t2i network, use pdm_uvit_t2i_forward");
  if (h->cfg.num_classes > 0 && !y) return fail(PDM_ERR_ARG, "pdm_uvit_forward: labels required (num_classes > 0)");
  if (h->cfg.num_classes <= 0 && y) return fail(PDM_ERR_ARG, "pdm_uvit_forward: labels given to an unconditional net");
  Workspace w;
  Ctx c;
  PDM_TRY(begin_forward(h, "pdm_uvit_forward", rows, workspace, workspace_bytes, stream, w, c));
  PDM_TRY(assemble_image(c, w, x, t, y, rows, h->Lx));
  PDM_TRY(run_stack(c, mode_of(h), w, rows, h->Lx));
  return run_tail(c, w, rows, final_norm(h, w, rows, h->Lx, h->n_patch), nullptr, 0, 0, eps_pre, nullptr);
}

int pdm_uvit_t2i_forward(pdm_uvit* h, const float* x, const float* t, const float* context, const float* mask_token,
                         int use_ground_truth, float* eps_pre, float* mask_pre, int rows, void* workspace,
                         size_t workspace_bytes, void* stream) {
  if (!h || !x || !t || !context || !eps_pre || rows <= 0) return fail(PDM_ERR_ARG, "pdm_uvit_t2i_forward: bad argument");
  if (!h->cfg.t2i) return fail(PDM_ERR_ARG, "pdm_uvit_t2i_forward: not a t2i network");
  if (mask_token && !h->cfg.enable_panoptic)
    return fail(PDM_ERR_ARG, "pdm_uvit_t2i_forward: mask tokens need a network built with enable_panoptic");
  if (mask_token && !use_ground_truth && !mask_pre)
    return fail(PDM_ERR_ARG, "pdm_uvit_t2i_forward: mask tokens without use_ground_truth need the mask_pre output");
  const bool joint = mask_token && !h->cfg.separate;  // one stack over [time, context, image patches, mask patches]
  Workspace w;
  Ctx c;
  PDM_TRY(begin_forward(h, "pdm_uvit_t2i_forward", rows, workspace, workspace_bytes, stream, w, c));
  const Mode m = mode_of(h);
  const int D = h->D, Lx = h->Lx, Lm = h->Lm, N = h->n_patch, nctx = h->cfg.num_clip_token, cd = h->cfg.clip_dim;
  {  // context_embed (libs/uvit_t2i.py:387): bf16 cast + GEMM (+bias) -> fp32 context tokens
    PDM_HIP(pdm::cast_bf16_launch(context, w.CTXB, (long long)rows * nctx * cd, c.s));
    pdm::GemmArgs a{};
    a.A1 = w.CTXB; a.lda1 = cd; a.K1 = cd;
    a.W = h->ctx_embed.w; a.bias = h->ctx_embed.bias;
    a.M = rows * nctx; a.N = D; a.K = cd;
    a.out_f32 = w.CTXF; a.ldr = D;
    a.stats_ld = a.ln_ld = (D + 255) / 256; a.ln_D = cd; a.ln_eps = 1e-5f;   // (carried, unused: no LayerNorm here)
    PDM_TRY(launch_gemm(c, a, pdm::EPI_F32));
  }
  PDM_TRY(assemble_image(c, w, x, t, nullptr, rows, joint ? Lm : Lx));
  if (mask_token && h->cfg.separate) {  // two block stacks with zero-conv injections
    // mask tokens m = mask_embed(mask_token) + pos_embed_mask (390, 406), stored at MX[:, Lx:Lm]
    PDM_TRY(assemble_mask(c, mask_token, h->pos_mask, w.MX, rows));
    return (m.r16 ? t2i_two_stream16 : t2i_two_stream32)(c, m, w, rows, use_ground_truth, eps_pre, mask_pre);
  }
  if (!joint) {  // plain text-conditioned U-ViT (mask_token None: 407-410, 516-517)
    PDM_TRY(run_stack(c, m, w, rows, Lx));
    return run_tail(c, w, rows, final_norm(h, w, rows, Lx, N), nullptr, 0, 0, eps_pre, nullptr);
  }
  // separate=False (397-399, 419-520): mask patches + pos_embed[Lx:Lm] -> rows [Lx, Lm) of X, the single stack over
  // all Lm rows, both heads on norm(x) of the 2N patch rows -> HEADIN [rows][2N][D]; with use_ground_truth the
  // image row and its mask row are normalised and summed in one pass -> HEADIN [rows][N][D]
  PDM_TRY(assemble_mask(c, mask_token, h->pos + (size_t)Lx * D, w.X, rows));
  PDM_TRY(run_stack(c, m, w, rows, Lm));
  pdm::LayerNormArgs ln = final_norm(h, w, rows, Lm, use_ground_truth ? N : 2 * N);
  if (use_ground_truth) ln.pair_offset = N;
  ln.add_ld = 0;   // (no added rows in this tail; it has always carried 0 here)
  return run_tail(c, w, rows, ln, use_ground_truth ? nullptr : w.HEADIN, 2 * N, N, eps_pre, mask_pre);
}

int pdm_stage_epilogue(const pdm_stage_epilogue_args* a, void* stream) {
  if (!a) return fail(PDM_ERR_ARG, "pdm_stage_epilogue: null args");
  pdm::EpilogueArgs e{};
  e.pre = a->pre; e.w = a->conv_w; e.bias = a->conv_b;
  e.B = a->B; e.C = a->C; e.Himg = a->H; e.Wimg = a->W;
  e.has_uncond = a->has_uncond; e.cfg_scale = a->cfg_scale;
  e.act_tanh = a->act_tanh;
  e.xin = a->xin; e.ax = a->ax; e.ae = a->ae;
  e.m_out = a->m_out;
  e.n_terms = a->n_terms;
  for (int i = 0; i < 6; ++i) { e.T[i] = a->T[i]; e.c[i] = a->c[i]; }
  e.cm = a->cm;
  e.x_out = a->x_out;
  e.x_out2 = a->x_out2;
  e.x_out3 = a->x_out3;
  PDM_CHECK(pdm::epilogue_check(e));
  PDM_HIP(pdm::epilogue_launch(e, (hipStream_t)stream));
  return PDM_OK;
}

int pdm_lincomb(float* out, int n_terms, const float* const* T, const float* c, long long n, void* stream) {
  if (!out || n_terms < 0 || n_terms > 8 || (n_terms && (!T || !c))) return fail(PDM_ERR_ARG, "pdm_lincomb: bad argument");
  PDM_HIP(pdm::lincomb_launch(out, n_terms, T, c, n, (hipStream_t)stream));
  return PDM_OK;
}

int pdm_gemm_bf16(const void* A1, int lda1, const void* A2, int lda2, int K1, const void* W, const float* bias, int M,
                  int N, int K, int epi, void* out_bf16, int ldo, float* out_f32, int ldr, int accumulate,
                  void* stream) {
  pdm::GemmArgs a{};
  a.A1 = (const bf16*)A1; a.lda1 = lda1;
  a.A2 = (const bf16*)A2; a.lda2 = lda2;
  a.K1 = A2 ? K1 : K;
  a.W = (const bf16*)W; a.bias = bias;
  a.M = M; a.N = N; a.K = K;
  a.out_bf16 = (bf16*)out_bf16; a.ldo = ldo;
  a.out_f32 = out_f32; a.ldr = ldr;
  a.accumulate = accumulate;
  PDM_CHECK(pdm::gemm_check(a, epi));
  PDM_HIP(pdm::gemm_launch(a, epi, (hipStream_t)stream));
  return PDM_OK;
}

int pdm_gemm_bf16_ln(const void* A, int lda, const void* W, const float* bias, int M, int N, int K, int epi,
                     void* out_bf16, int ldo, float* out_f32, int ldr, int accumulate, float* stats_out,
                     const float* ln_stats, const float* ln_colsum, float ln_eps, void* stream) {
  pdm::GemmArgs a{};
  a.A1 = (const bf16*)A; a.lda1 = lda; a.K1 = K;
  a.W = (const bf16*)W; a.bias = bias;
  a.M = M; a.N = N; a.K = K;
  a.out_bf16 = (bf16*)out_bf16; a.ldo = ldo;
  a.out_f32 = out_f32; a.ldr = ldr;
  a.accumulate = accumulate;
  a.stats_out = stats_out; a.stats_ld = (N + 255) / 256;
  a.ln_stats = ln_stats; a.ln_ld = (K + 255) / 256; a.ln_D = K; a.ln_eps = ln_eps; a.ln_colsum = ln_colsum;
  PDM_CHECK(pdm::gemm_check(a, epi));
  PDM_HIP(pdm::gemm_launch(a, epi, (hipStream_t)stream));
  return PDM_OK;
}

int pdm_rowstats(const float* x, int ldx, int rows, int D, void* xb, float* stats, void* stream) {
  if (!x || !stats || rows <= 0 || D <= 0 || D % 4 || D > 2048) return fail(PDM_ERR_ARG, "pdm_rowstats: bad argument");
  PDM_HIP(pdm::rowstats_launch(x, ldx, rows, D, (bf16*)xb, D, stats, (D + 255) / 256, (hipStream_t)stream));
  return PDM_OK;
}

// stream-K state for standalone pdm_gemm calls (pdm_set_gemm_sk mode bit 2; tests and tools): the calling stream's
// ring (sk_state), its next flag block per call, the ring zeroed on the stream whenever it wraps
static int sk_standalone(pdm::GemmArgs& a, hipStream_t s) {
  SkState* st = nullptr;
  PDM_TRY(sk_state(s, &st));
  if (!st) return PDM_OK;   // capturing without a state: whole tiles
  if (st->next == SK_RING) {
    PDM_HIP(hipMemsetAsync(st->flags, 0, (size_t)SK_RING * pdm::SK_FLAG_WORDS * 4, s));
    st->next = 0;
  }
  a.sk_flags = st->flags + (size_t)st->next++ * pdm::SK_FLAG_WORDS;
  a.sk_slab = st->slab;
  return PDM_OK;
}

static pdm::GemmArgs to_gemm_args(const pdm_gemm_args* g) {
  pdm::GemmArgs a{};
  a.A1 = (const bf16*)g->A1; a.lda1 = g->lda1;
  a.A2 = (const bf16*)g->A2; a.lda2 = g->lda2;
  a.K1 = g->A2 ? g->K1 : g->K;
  a.W = (const bf16*)g->W; a.ldw = g->ldw; a.bias = g->bias;
  a.M = g->M; a.N = g->N; a.K = g->K;
  a.out_bf16 = (bf16*)g->out_bf16; a.ldo = g->ldo;
  a.out_f32 = g->out_f32; a.ldr = g->ldr; a.accumulate = g->accumulate;
  a.stats_out = g->stats_out; a.stats_ld = (g->N + 255) / 256;
  a.ln_stats = g->ln_stats; a.ln_ld = (g->K + 255) / 256; a.ln_D = g->K; a.ln_eps = g->ln_eps; a.ln_colsum = g->ln_colsum;
  a.fp8 = g->fp8;
  a.a_scale = g->a_scale; a.a_scale_ld = g->a_scale_ld;
  a.w_scale = g->w_scale; a.w_scale_ld = g->w_scale_ld;
  a.out_fp8 = (unsigned char*)g->out_fp8; a.ldo8 = g->ldo8;
  a.out_scale = g->out_scale; a.out_scale_ld = g->out_scale_ld;
  a.mx_center = g->mx_center; a.ln_gcol = (const bf16*)g->ln_gcol;
  a.res_in = (const bf16*)g->res_in; a.ldri = g->ldri;
  a.res_f32 = g->res_f32; a.ldrf = g->ldrf;
  a.a_rows_per_group = g->a_rows_per_group; a.a_group_stride = g->a_group_stride;
  a.out2 = (bf16*)g->out2; a.out2_rpg = g->out2_rows_per_group; a.out2_gs = g->out2_group_stride;
  a.stats_out2 = g->stats_out2;
  return a;
}

int pdm_gemm(const pdm_gemm_args* g, int epi, void* stream) {
  if (!g) return fail(PDM_ERR_ARG, "pdm_gemm: null args");
  pdm::GemmArgs a = to_gemm_args(g);
  PDM_CHECK(pdm::gemm_check(a, epi));
  if (g_sk_standalone) PDM_TRY(sk_standalone(a, (hipStream_t)stream));
  PDM_HIP(pdm::gemm_launch(a, epi, (hipStream_t)stream));
  return PDM_OK;
}

int pdm_gemm_pair(const pdm_gemm_args* ga, const pdm_gemm_args* gb, int epi, void* stream) {
  if (!ga || !gb) return fail(PDM_ERR_ARG, "pdm_gemm_pair: null args");
  const pdm::GemmArgs a = to_gemm_args(ga), b = to_gemm_args(gb);
  PDM_CHECK(pdm::gemm_check(a, epi));
  PDM_CHECK(pdm::gemm_check(b, epi));
  PDM_HIP(pdm::gemm_launch_pair(a, b, epi, (hipStream_t)stream));
  return PDM_OK;
}

int pdm_gemm_args_size(void) { return (int)sizeof(pdm_gemm_args); }

// the GemmArgs pdm_gemm builds, with the launch options pdm_gemm_args lacks; stand-in addresses (never dereferenced)
// for the operands the options imply
static pdm::GemmArgs to_plan_args(const pdm_gemm_args* g, const pdm_gemm_plan_opts* o) {
  pdm::GemmArgs a = to_gemm_args(g);
  void* const stand_in = (void*)(uintptr_t)4096;
  if (o->convC > 0) {
    a.conv = 1; a.convH = o->convH; a.convW = o->convW; a.convC = o->convC; a.conv_up = o->conv_up;
    a.zero = (const bf16*)stand_in;
  }
  a.batch = o->batch;
  a.act = o->act;
  if (o->gn_P > 0) { a.gn_part = (double*)stand_in; a.gn_P = o->gn_P; a.gn_cpg = a.N / 32; }
  if (o->sk_attached) { a.sk_flags = (unsigned*)stand_in; a.sk_slab = (float*)stand_in; }
  return a;
}

int pdm_gemm_plan(const pdm_gemm_args* ga, const pdm_gemm_args* gb, int epi, const pdm_gemm_plan_opts* o, int* out24) {
  if (!ga || !o || !out24) return fail(PDM_ERR_ARG, "pdm_gemm_plan: null argument");
  if (o->algo > 11 || o->algo == 10 || (o->sk_mode > 2) || o->raster > 64)
    return fail(PDM_ERR_ARG, "pdm_gemm_plan: algo must be 0..9 or 11, sk_mode 0..2, raster <= 64 (negative: current)");
  const pdm::GemmArgs a = to_plan_args(ga, o);
  PDM_CHECK(pdm::gemm_check(a, epi));
  pdm::GemmPolicy pol = pdm::gemm_policy(o->ncu > 0 ? o->ncu : -1, o->persist_ok);
  if (o->algo >= 0) pol.algo = o->algo;
  if (o->sk_mode >= 0) pol.sk = o->sk_mode;
  if (o->raster >= 0) pol.raster = o->raster;
  if (o->dbg >= 0) pol.dbg = o->dbg;
  if (o->mx_res_persist >= 0) pol.mx_res_persist = o->mx_res_persist;
  pdm::GemmPlan pl{};
  bool grouped = false;
  if (gb) {
    const pdm::GemmArgs b = to_plan_args(gb, o);
    PDM_CHECK(pdm::gemm_check(b, epi));
    grouped = pdm::gemm_plan_pair(a, b, epi, pol, &pl);
  }
  if (!grouped) {
    pdm::GemmArgs one = a;
    if (gb) one.sk_flags = nullptr, one.sk_slab = nullptr;   // pdm_gemm_pair: one flag block serves one launch
    pl = pdm::gemm_plan(one, epi, pol);
  }
  const int v[24] = {pl.error, pl.family, pl.epi, pl.conv, pl.sched, pl.mxo, pl.sk, pl.fp8, pl.dual, pl.grid_x, pl.grid_y,
                     pl.block, pl.lds_bytes, pl.tiles_n, pl.ntiles, pl.nt0, pl.raster, pl.split_m1, pl.rowstats,
                     pl.out2_copy, pl.writes_gn, pdm::gemm_gn_fusable(a, epi, pol), grouped, pl.kernel};
  for (int i = 0; i < 24; ++i) out24[i] = v[i];
  return PDM_OK;
}

int pdm_gemm_conv3x3_bf16(const void* in, int B, int H, int W, int Cin, int up, const void* Wt, const float* bias,
                          int N, int epi, void* out_bf16, float* out_f32, int accumulate, void* stream) {
  static bf16* zero = nullptr;   // zero page for the tile policies that address padded taps explicitly
  if (!zero) {
    PDM_HIP(hipMalloc(&zero, 4096));
    PDM_HIP(hipMemset(zero, 0, 4096));
  }
  pdm::GemmArgs a{};
  a.A1 = (const bf16*)in; a.lda1 = Cin; a.K1 = 9 * Cin;
  a.W = (const bf16*)Wt; a.bias = bias;
  a.M = B * H * W; a.N = N; a.K = 9 * Cin;
  a.out_bf16 = (bf16*)out_bf16; a.ldo = N;
  a.out_f32 = out_f32; a.ldr = N;
  a.accumulate = accumulate;
  a.conv = 1; a.convH = H; a.convW = W; a.convC = Cin; a.conv_up = up; a.zero = zero;
  PDM_CHECK(pdm::gemm_check(a, epi));
  PDM_HIP(pdm::gemm_launch(a, epi, (hipStream_t)stream));
  return PDM_OK;
}

int pdm_gemm_batched_bf16(const void* A, int lda, long long sA, const void* W, int ldw, long long sW,
                          const float* bias, int M, int N, int K, int batch, int epi, void* out_bf16, int ldo,
                          long long sO, float* out_f32, int ldr, long long sR, int accumulate, void* stream) {
  pdm::GemmArgs a{};
  a.A1 = (const bf16*)A; a.lda1 = lda; a.K1 = K;
  a.W = (const bf16*)W; a.ldw = ldw; a.bias = bias;
  a.M = M; a.N = N; a.K = K;
  a.out_bf16 = (bf16*)out_bf16; a.ldo = ldo;
  a.out_f32 = out_f32; a.ldr = ldr;
  a.accumulate = accumulate;
  a.batch = batch; a.sA = sA; a.sW = sW; a.sO = sO; a.sR = sR;
  if (batch < 1) return fail(PDM_ERR_ARG, "pdm_gemm_batched_bf16: batch must be >= 1");
  PDM_CHECK(pdm::gemm_check(a, epi));
  PDM_HIP(pdm::gemm_launch(a, epi, (hipStream_t)stream));
  return PDM_OK;
}

int pdm_layernorm(const float* x, int ldx, const float* gamma, const float* beta, void* y, int ldy, int rows, int D,
                  float eps, void* stream) {
  pdm::LayerNormArgs a{};
  a.x = x; a.ldx = ldx; a.gamma = gamma; a.beta = beta; a.y = (bf16*)y; a.ldy = ldy;
  a.rows = rows; a.D = D; a.rows_per_group = 1; a.group_stride = 1; a.row_offset = 0; a.eps = eps;
  PDM_CHECK(pdm::layernorm_check(a));
  PDM_HIP(pdm::layernorm_launch(a, (hipStream_t)stream));
  return PDM_OK;
}

int pdm_attention(const void* qkv, int ldq, void* out, int ldo, int B, int L, int H, int Dh, float scale,
                  void* stream) {
  pdm::AttentionArgs a{};
  a.qkv = (const bf16*)qkv; a.ldq = ldq; a.out = (bf16*)out; a.ldo = ldo;
  a.B = B; a.L = L; a.H = H; a.Dh = Dh; a.scale = scale;
  PDM_CHECK(pdm::attention_check(a));
  PDM_HIP(pdm::attention_launch(a, (hipStream_t)stream));
  return PDM_OK;
}

int pdm_attention_log2(const void* qkv, int ldq, void* out, int ldo, int B, int L, int H, int Dh, void* stream) {
  pdm::AttentionArgs a{};
  a.qkv = (const bf16*)qkv; a.ldq = ldq; a.out = (bf16*)out; a.ldo = ldo;
  a.B = B; a.L = L; a.H = H; a.Dh = Dh; a.scale = 1.0f / sqrtf((float)Dh); a.q_log2 = 1;
  PDM_CHECK(pdm::attention_check(a));
  PDM_HIP(pdm::attention_launch(a, (hipStream_t)stream));
  return PDM_OK;
}

int pdm_mx_quantize(const void* x, int dtype, int ldx, int rows, int K, void* q, int ldq, unsigned* s, int s_ld,
                    void* stream) {
  if (dtype != PDM_F32 && dtype != PDM_BF16) return fail(PDM_ERR_ARG, "pdm_mx_quantize: dtype must be PDM_F32 or PDM_BF16");
  const hipError_t e = pdm::mxq_launch(x, dtype == PDM_F32 ? 0 : 1, ldx, rows, K, (unsigned char*)q, ldq, s, s_ld,
                                       (hipStream_t)stream);
  if (e == hipErrorInvalidValue)
    return fail(PDM_ERR_ARG, "pdm_mx_quantize: K % 32, ldx / ldq >= K, s_ld >= rows and 16-byte aligned rows required");
  PDM_HIP(e);
  return PDM_OK;
}

int pdm_f32_to_bf16(const float* x, void* y, long long n, void* stream) {
  if (n == 0) return PDM_OK;   // empty tensors may carry null data pointers
  if (!x || !y || n < 0) return fail(PDM_ERR_ARG, "pdm_f32_to_bf16: bad argument");
  PDM_HIP(pdm::cast_bf16_launch(x, (bf16*)y, n, (hipStream_t)stream));
  return PDM_OK;
}

}  // extern "C"
