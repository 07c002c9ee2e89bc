// libafx engine: weight store + forward orchestration + the C ABI of include/afx.h
// (but for the streaming kernels' entry points, defined beside their kernels).
// Host code (C++) over the HIP runtime; the only device code here is a few one-off
// weight-preparation kernels.  The forward is a fixed sequence of asynchronous kernel
// launches on the caller's stream: no allocation, no synchronisation, no host<->device
// copies inside afx_forward (it can be captured into a hipGraph by the caller).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../include/afx.h"
#include "afx_common.h"
#include "afx_kernels.h"
#include "afx_aasist.h"
#include "afx_entry.h"

using namespace afx;

// ---------------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------------
static thread_local char g_err[512] = "";
int afx::fail(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return 1;
}
#define HIP_OK(expr)                                                               \
  do {                                                                             \
    hipError_t e_ = (expr);                                                        \
    if (e_ != hipSuccess) return fail("%s: %s", #expr, hipGetErrorString(e_));     \
  } while (0)
#define KOK(expr)                                    \
  do {                                               \
    const char* m_ = (expr);                         \
    if (m_) return fail("%s", m_);                   \
  } while (0)

// ---------------------------------------------------------------------------------
// model constants (XLS-R 300M trunk)
// ---------------------------------------------------------------------------------
static const int kConvK[7] = {10, 3, 3, 3, 3, 2, 2};
static const int kConvS[7] = {5, 2, 2, 2, 2, 2, 2};
constexpr int kC = 512;      // conv channels
constexpr int kD = 1024;     // encoder width
constexpr int kF = 4096;     // FFN width
constexpr int kH = 16;       // heads
constexpr int kPosK = 128;   // positional conv taps
constexpr int kPosG = 16;    // positional conv groups
constexpr int kPosPad = 64;  // = kPosK / 2
constexpr float kLnEps = 1e-5f;
constexpr float kBnEps = 1e-5f;

static int round_up(int v, int m) { return (v + m - 1) / m * m; }

static void conv_lengths(int L, int* T) {
  for (int i = 0; i < 7; ++i) {
    L = L >= kConvK[i] ? (L - kConvK[i]) / kConvS[i] + 1 : 0;
    T[i] = L;
  }
}

// one-off device helpers ------------------------------------------------------------
__global__ void bn_fold_kernel(const float* w, const float* b, const float* m, const float* v, float eps, int n,
                               float* scale, float* shift) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const float s = w[i] / sqrtf(v[i] + eps);
    scale[i] = s;
    shift[i] = b[i] - m[i] * s;
  }
}

__global__ void absmax_kernel(const float* x, int n, float* out) {  // out[0] = max |x| (one workgroup)
  float m = 0.f;
  for (int i = threadIdx.x; i < n; i += blockDim.x) m = fmaxf(m, fabsf(x[i]));
  __shared__ float red[4];
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

struct FT {  // fp32 device tensor owned by the engine
  float* p = nullptr;
  size_t n = 0;
  std::vector<int64_t> shape;
};

struct TapRec {
  float* p = nullptr;  // engine-owned fp32 copy
  size_t cap = 0, n = 0;
};

// The weight tables.  afx_create allocates the packed operands; resolve_weights (run by every afx_finalize) fills in every raw
// fp32 tensor a launch reads, checked for presence and element count.  The launch paths read these fields and nothing else.
struct LnW {  // a LayerNorm the engine launches
  const float *g = nullptr, *b = nullptr;
  // split precision: the scale its output takes as a pair-form operand, chosen at finalize (s3_layernorm_scales) from
  // |y| <= sqrt(C) max|gamma| + max|beta|: the largest power of two <= kS3ScaleBounded that keeps the hi half inside fp16 -- a
  // LayerNorm output cannot overflow whatever the checkpoint's gains are
  float scale = kS3ScaleBounded;
};
struct ConvLayer {  // conv feature encoder, layer 0..6 (the packed weights of layers 1-6: afx_engine::convw)
  const float* bias = nullptr;  // group-norm mode: null (bias-free convs)
  LnW ln;                       // layer_norm mode
  const float *w0 = nullptr, *gn_g = nullptr, *gn_b = nullptr;  // layer 0: fp32 weight; group-norm mode: GroupNorm(512,512)
};
struct TrunkLayer {
  void *wqkv = nullptr, *wo = nullptr, *w1 = nullptr, *w2 = nullptr;  // packed operands
  float* bqkv = nullptr;
  LnW ln1, ln2;  // self_attn_layer_norm, final_layer_norm
  const float *bo = nullptr, *b1 = nullptr, *b2 = nullptr;
};
struct ConfFF {
  void *w1, *w2;
  LnW ln;
  const float *b1, *b2;
};
struct ConfBlock {
  ConfFF ff[2];
  void *wqkv, *wout, *pw1, *pw2;
  float *bn_scale, *bn_shift;
  void* rel_h;          // rel_pos_emb in operand type, rows padded to 64 (matrix-core attention)
  float* chain_prm[3];  // per fused chain: the per-column vectors packed into one 8-KB block (ConfChainArgs::params)
  // what the per-op path and the fp32 VALU kernels read
  LnW attn_ln, conv_ln, post_ln;
  const float *bout, *bpw1, *bpw2;
  const float* rel32;  // rel_pos_emb (1025, dh)
  const float *dw_w, *dw_b;
};

struct Profiler;  // per-engine launch timing (below)

struct afx_engine {
  afx_config cfg;
  bool s3 = false;  // split precision (AFX_DT_FP16X3): dt == DT_FP32 for every kernel but the dense products
  Profiler* prof = nullptr;  // owned; no process-wide map: two engines on two host threads share nothing
  int dt;
  size_t hsz;  // bytes per operand element
  std::vector<void*> allocs;
  std::unordered_map<std::string, FT> f;  // raw fp32 tensors by canonical name
  std::unordered_set<std::string> loaded;
  bool finalized = false;
  bool taps_on = false;
  // A/B switches between forms of the same op (afx_engine_set; per engine: another engine of the process is not touched)
  int posconv_sliding = 1;  // positional conv: sliding-window kernel (0: chunked-K GEMM)
  int conf_attn_mfma = 1;   // Conformer attention on the matrix cores (0: the fp32 VALU kernel)
  int fuse_conformer = 1;   // Conformer block: row-local chains fused (afx_conformer_fused.hip); 0 = per-op path
  int fuse_conv_ln = 1;     // conv layers 1-6: LayerNorm + GELU in the GEMM epilogue (0: two kernels)
  int gemm_small_deep = 1;  // products with at most two 128x64 tiles per CU: the deep form of that tile (0: the two-buffer form)
  int concurrent = 0;  // 1: the calls that follow run beside another forward on a second stream -- launch shapes by CU time (OBJ_CU_TIME)
  int last_objective = 0;  // the objective the last native call on this handle ran under (afx_engine_get "objective")
  std::unordered_map<std::string, TapRec> taps;
  // overflow guard: device counters [0] rows of the trunk's final LayerNorm with non-finite statistics, [1] non-finite logits
  // (written by those kernels of every forward, read and cleared by afx_check_finite)
  int* nonfinite = nullptr;

  // trunk: packed operand-type weights, and the raw tensors resolve_weights found
  void* convw[7] = {nullptr};
  void* conv0pack = nullptr;  // layer 0 as the split-precision fp16 MFMA operand (layer_norm mode, half-precision engines)
  void* projw = nullptr;
  void* posw = nullptr;
  float* pos_norm = nullptr;
  ConvLayer conv[7];
  LnW feat_ln, enc_ln;  // layer_norm, encoder.layer_norm
  const float *proj_b = nullptr, *pos_b = nullptr;
  std::vector<TrunkLayer> layers;
  // Conformer head
  int E = 0, Ep = 0, heads = 0, dh = 0, inner = 0, FF = 0, FFp = 0, C2 = 0, C2p = 0, ck = 0, nblk = 0;
  void* conf_ll = nullptr;
  float conf_bn_scale = 1.f, conf_bn_shift = 0.f;
  const float *ll_b = nullptr, *class_token = nullptr, *fc5_w = nullptr, *fc5_b = nullptr;
  std::vector<ConfBlock> blk;
  // AASIST head
  AasistWeights aw;

  // a packed weight matrix [rows][k] (+, in split precision, its per-row scales behind it: wscale())
  void* walloc(size_t rows, size_t k) { return dalloc(rows * k * hsz + (s3 ? rows * 4 : 0)); }
  float* wscale(const void* w, size_t rows, size_t k) const { return s3 ? (float*)((char*)w + rows * k * 4) : nullptr; }
  void* dalloc(size_t bytes) {
    void* p = nullptr;
    if (hipMalloc(&p, bytes ? bytes : 16) != hipSuccess) return nullptr;
    allocs.push_back(p);
    return p;
  }
  const float* F(const std::string& k) const {
    auto it = f.find(k);
    return it == f.end() ? nullptr : it->second.p;
  }
};

// ---------------------------------------------------------------------------------
// lifecycle
// ---------------------------------------------------------------------------------
static void prof_forget(afx_engine* e);
extern "C" const char* afx_last_error(void) { return g_err; }
extern "C" const char afx_build_id_str[];  // build_id.gen.c (Makefile): hash of the sources this library was built from
extern "C" const char* afx_build_id(void) { return afx_build_id_str; }
extern "C" const char* afx_version(void) {
  static char v[96] = "";
  if (!v[0]) snprintf(v, sizeof v, "afx 0.4 (gfx950) build %s hip %d.%d.%d", afx_build_id_str, HIP_VERSION_MAJOR, HIP_VERSION_MINOR, HIP_VERSION_PATCH);
  return v;
}
// The HIP version the library's code objects and launch stubs were compiled against, and the version of the runtime this
// process actually resolved (a torch wheel bundles its own libamdhip64; afx/_lib.py loads torch first so that the process has
// ONE runtime): the host side refuses a different major version and warns when the runtime is older than the toolchain.
extern "C" int afx_hip_versions(int* build, int* runtime) {
  if (build) *build = HIP_VERSION;
  int rt = 0;
  if (hipRuntimeGetVersion(&rt) != hipSuccess) return fail("afx_hip_versions: hipRuntimeGetVersion failed");
  if (runtime) *runtime = rt;
  return 0;
}

extern "C" int afx_create(const afx_config* cfg, afx_handle* out) {
  if (!cfg || !out) return fail("afx_create: null argument");
  const bool head_only = cfg->arch == AFX_ARCH_CONFORMER_HEAD;  // MyConformer alone: no trunk in this handle
  if (!head_only && (cfg->n_layers < 1 || cfg->n_layers > 24))
    return fail("Number of layers must be at least 1 and at most 24.");  // models/fe.py:60-62
  if (cfg->dtype != AFX_DT_BF16 && cfg->dtype != AFX_DT_FP16 && cfg->dtype != AFX_DT_FP32 && cfg->dtype != AFX_DT_FP16X3)
    return fail("afx_create: unknown dtype %d", cfg->dtype);
  if (cfg->arch < AFX_ARCH_SSL || cfg->arch > AFX_ARCH_CONFORMER_HEAD) return fail("afx_create: unknown arch %d", cfg->arch);
  if (cfg->extractor_mode != AFX_EXTRACTOR_LAYER_NORM && cfg->extractor_mode != AFX_EXTRACTOR_GROUP_NORM)
    return fail("afx_create: unknown extractor_mode %d", cfg->extractor_mode);
  if (cfg->extractor_mode == AFX_EXTRACTOR_GROUP_NORM && cfg->pre_emphasis)
    return fail("afx_create: fused pre-emphasis is built for the layer_norm extractor only");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail("afx_create: no HIP device visible -- this library has no CPU fallback");
  afx_engine* e = new afx_engine();
  e->cfg = *cfg;
  // split precision: activations and every non-GEMM kernel as in exact mode (fp32); the dense products on the fp16 matrix
  // pipe with hi / lo operand pairs (Call::gemm below).  A weight element is 4 bytes either way (fp32, or an fp16 hi + lo pair).
  e->s3 = cfg->dtype == AFX_DT_FP16X3;
  e->dt = e->s3 ? (int)DT_FP32 : cfg->dtype;
  e->hsz = dtype_size(e->dt);
  const int nl = head_only ? 0 : cfg->n_layers;
  e->cfg.n_layers = nl;
  e->layers.resize(nl);
  bool ok = true;
  ok &= (e->nonfinite = (int*)e->dalloc(16)) != nullptr && hipMemset(e->nonfinite, 0, 16) == hipSuccess;
  if (!head_only) {
    for (int i = 1; i < 7; ++i) ok &= (e->convw[i] = e->walloc(kC, (size_t)kC * kConvK[i])) != nullptr;
    ok &= (e->projw = e->walloc(kD, kC)) != nullptr;
    ok &= (e->posw = e->walloc(kD, (size_t)(kD / kPosG) * kPosK)) != nullptr;
    ok &= (e->pos_norm = (float*)e->dalloc(kPosK * 4)) != nullptr;
  }
  for (int l = 0; l < nl && ok; ++l) {
    TrunkLayer& t = e->layers[l];
    ok &= (t.wqkv = e->walloc(3 * kD, kD)) != nullptr;
    ok &= (t.wo = e->walloc(kD, kD)) != nullptr;
    ok &= (t.w1 = e->walloc(kF, kD)) != nullptr;
    ok &= (t.w2 = e->walloc(kD, kF)) != nullptr;
    ok &= (t.bqkv = (float*)e->dalloc((size_t)3 * kD * 4)) != nullptr;
  }
  if (cfg->arch == AFX_ARCH_CONFORMER || head_only) {
    e->E = cfg->conf_emb;
    e->heads = cfg->conf_heads;
    e->ck = cfg->conf_kernel;
    e->nblk = cfg->conf_blocks;
    if (e->E <= 0 || e->heads <= 0 || e->E % e->heads || e->E % 4 || e->ck <= 0 || e->nblk <= 0) {
      afx_destroy(e);  // (the message reads the caller's cfg: `e` is gone -- a use-after-free found by `make asan`)
      return fail("afx_create: bad Conformer configuration (emb %d heads %d kernel %d blocks %d)", cfg->conf_emb, cfg->conf_heads,
                  cfg->conf_kernel, cfg->conf_blocks);
    }
    e->dh = e->E / e->heads;
    e->inner = e->dh * e->heads;
    e->Ep = round_up(e->E, 64);
    e->FF = 4 * e->E;
    e->FFp = round_up(e->FF, 64);
    e->C2 = 2 * e->E;
    e->C2p = round_up(e->C2, 64);
    if (!head_only) ok &= (e->conf_ll = e->walloc(e->E, kD)) != nullptr;
    e->blk.resize(e->nblk);
    for (int b = 0; b < e->nblk && ok; ++b) {
      ConfBlock& B = e->blk[b];
      for (ConfFF& ff : B.ff) {
        ok &= (ff.w1 = e->walloc(e->FF, e->Ep)) != nullptr;
        ok &= (ff.w2 = e->walloc(e->E, e->FFp)) != nullptr;
      }
      ok &= (B.wqkv = e->walloc(3 * e->inner, e->Ep)) != nullptr;
      ok &= (B.wout = e->walloc(e->E, e->Ep)) != nullptr;
      ok &= (B.pw1 = e->walloc(2 * e->C2, e->Ep)) != nullptr;
      ok &= (B.pw2 = e->walloc(e->E, e->C2p)) != nullptr;
      ok &= (B.bn_scale = (float*)e->dalloc((size_t)e->C2 * 4)) != nullptr;
      ok &= (B.bn_shift = (float*)e->dalloc((size_t)e->C2 * 4)) != nullptr;
      for (int st = 0; st < 3; ++st) ok &= (B.chain_prm[st] = (float*)e->dalloc((kChainParamFloats + kChainScaleFloats) * 4)) != nullptr;
      ok &= (B.rel_h = e->dalloc((size_t)1025 * 64 * e->hsz)) != nullptr;
    }
  }
  if (!ok) {
    afx_destroy(e);
    return fail("afx_create: device allocation failed");
  }
  *out = e;
  return 0;
}

extern "C" void afx_destroy(afx_handle h) {
  if (!h) return;
  prof_forget(h);
  for (void* p : h->allocs) (void)hipFree(p);
  for (auto& t : h->taps)
    if (t.second.p) (void)hipFree(t.second.p);
  delete h;
}

extern "C" int afx_enable_taps(afx_handle h, int on) {
  if (!h) return fail("afx_enable_taps: null handle");
  h->taps_on = on != 0;
  return 0;
}

// Overflow guard.  The half-precision modes keep operand COPIES in fp16 / bf16 (LayerNorm outputs, q | k | v rows, attention
// output, the GELU'd FFN hidden, conv-stack activations; split precision: fp16 hi / lo pairs of scale x the value).  A
// trained checkpoint with outlier channels can push one of them past the format's range (fp16: 65 504; fp16x3: 65 504 /
// its activation scale: kS3ScaleFree = 1 for unbounded operands); the inf then turns every later row statistic into NaN.  Rather than hand back NaN -- or, behind the AASIST
// head's max-pooling and top-k, finite garbage -- scores, the trunk's final LayerNorm and the kernels that write the logits
// count what is not finite (no cost: one compare per row / logit), and this call turns a non-zero count into an error:
// it waits for `stream`, reads and clears the counters.  Scoring loops call it once, before they write a score.
extern "C" int afx_check_finite(afx_handle h, void* stream) {
  if (!h) return fail("afx_check_finite: null handle");
  int c[2] = {0, 0};
  hipStream_t s = (hipStream_t)stream;
  HIP_OK(hipMemcpyAsync(c, h->nonfinite, 8, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  if (c[0] || c[1]) {
    HIP_OK(hipMemsetAsync(h->nonfinite, 0, 8, s));
    return fail("non-finite values since the last check: %d feature rows of the trunk's final LayerNorm, %d logits -- an operand copy left the "
                "range of this engine's precision (%s); the scores of these batches are invalid.  Use dtype \"fp32\" (exact mode) for this checkpoint",
                c[0], c[1], h->s3 ? "fp16x3: fp16 hi / lo pairs" : (h->dt == AFX_DT_FP16 ? "fp16 operands: |x| <= 65504" : (h->dt == AFX_DT_BF16 ? "bf16 operands" : "fp32")));
  }
  return 0;
}

// ---------------------------------------------------------------------------------
// weights
// ---------------------------------------------------------------------------------
static bool starts_with(const std::string& s, const char* p) { return s.compare(0, strlen(p), p) == 0; }
static bool ends_with(const std::string& s, const char* p) {
  const size_t n = strlen(p);
  return s.size() >= n && s.compare(s.size() - n, n, p) == 0;
}
static size_t numel(const int64_t* shape, int ndim) {
  size_t n = 1;
  for (int i = 0; i < ndim; ++i) n *= (size_t)shape[i];
  return n;
}
static int expect_shape(const char* name, const int64_t* shape, int ndim, std::initializer_list<int64_t> want) {
  size_t have = numel(shape, ndim), w = 1;
  for (int64_t v : want) w *= (size_t)v;
  if (have != w) return fail("afx_load_weight: %s has %zu elements, expected %zu", name, have, w);
  return 0;
}

static int store_raw(afx_engine* e, const std::string& key, const float* src, const int64_t* shape, int ndim,
                     hipStream_t s) {
  FT& t = e->f[key];
  const size_t n = numel(shape, ndim);
  if (!t.p || t.n != n) {
    if (t.p) {  // reloaded with another size: release the old buffer now, not at destroy
      for (auto it = e->allocs.begin(); it != e->allocs.end(); ++it)
        if (*it == t.p) { e->allocs.erase(it); break; }
      (void)hipFree(t.p);
    }
    t.p = (float*)e->dalloc(n * 4);
    if (!t.p) return fail("afx_load_weight: device allocation failed for %s", key.c_str());
    t.n = n;
  }
  t.shape.assign(shape, shape + ndim);
  HIP_OK(hipMemcpyAsync(t.p, src, n * 4, hipMemcpyDeviceToDevice, s));
  return 0;
}

// pack a weight into the engine's operand form; split precision: fp32 rows first, then hi / lo pairs + row scales in place
static const char* pack_linear(afx_engine* e, const float* src, int N, int K, int Kpad, void* dst, float* scale, hipStream_t s) {
  if (const char* m = launch_pack_linear(src, N, K, Kpad, dst, e->dt, s)) return m;
  return e->s3 ? launch_split_weight_rows(dst, N, Kpad, scale, s) : nullptr;
}

// trunk tensor (name without the "ssl_model.model." prefix)
static int load_ssl(afx_engine* e, const std::string& k, const float* src, const int64_t* shape, int ndim,
                    hipStream_t s) {
  int i = 0, n = 0;
  char tail[96];
  if (sscanf(k.c_str(), "feature_extractor.conv_layers.%d.%95s", &i, tail) == 2 && !strcmp(tail, "0.weight")) {
    if (i < 0 || i > 6) return fail("afx_load_weight: conv layer %d out of range", i);
    if (i == 0) {
      if (expect_shape(k.c_str(), shape, ndim, {kC, 1, kConvK[0]})) return 1;
      return store_raw(e, "ssl." + k, src, shape, ndim, s);
    }
    if (expect_shape(k.c_str(), shape, ndim, {kC, kC, kConvK[i]})) return 1;
    KOK(launch_pack_conv(src, kC, kC, kConvK[i], e->convw[i], e->dt, s));
    if (e->s3) KOK(launch_split_weight_rows(e->convw[i], kC, kC * kConvK[i], e->wscale(e->convw[i], kC, (size_t)kC * kConvK[i]), s));
    return 0;
  }
  if (k == "post_extract_proj.weight") {
    if (expect_shape(k.c_str(), shape, ndim, {kD, kC})) return 1;
    KOK(pack_linear(e, src, kD, kC, kC, e->projw, e->wscale(e->projw, kD, kC), s));
    return 0;
  }
  if (sscanf(k.c_str(), "encoder.layers.%d.%95s", &n, tail) == 2) {
    if (n < 0) return fail("afx_load_weight: bad layer index in %s", k.c_str());
    if (n >= e->cfg.n_layers) return 0;  // a deeper checkpoint than this (truncated) trunk keeps: ignore
    const std::string t = tail;
    static const char* proj[3] = {"self_attn.q_proj.", "self_attn.k_proj.", "self_attn.v_proj."};
    for (int j = 0; j < 3; ++j) {
      if (t == std::string(proj[j]) + "weight") {
        if (expect_shape(k.c_str(), shape, ndim, {kD, kD})) return 1;
        KOK(pack_linear(e, src, kD, kD, kD, (char*)e->layers[n].wqkv + (size_t)j * kD * kD * e->hsz,
                        e->s3 ? e->wscale(e->layers[n].wqkv, 3 * kD, kD) + j * kD : nullptr, s));
        return 0;
      }
      if (t == std::string(proj[j]) + "bias") {
        if (expect_shape(k.c_str(), shape, ndim, {kD})) return 1;
        HIP_OK(hipMemcpyAsync(e->layers[n].bqkv + j * kD, src, kD * 4, hipMemcpyDeviceToDevice, s));
        return 0;
      }
    }
    if (t == "self_attn.out_proj.weight") {
      if (expect_shape(k.c_str(), shape, ndim, {kD, kD})) return 1;
      KOK(pack_linear(e, src, kD, kD, kD, e->layers[n].wo, e->wscale(e->layers[n].wo, kD, kD), s));
      return 0;
    }
    if (t == "fc1.weight") {
      if (expect_shape(k.c_str(), shape, ndim, {kF, kD})) return 1;
      KOK(pack_linear(e, src, kF, kD, kD, e->layers[n].w1, e->wscale(e->layers[n].w1, kF, kD), s));
      return 0;
    }
    if (t == "fc2.weight") {
      if (expect_shape(k.c_str(), shape, ndim, {kD, kF})) return 1;
      KOK(pack_linear(e, src, kD, kF, kF, e->layers[n].w2, e->wscale(e->layers[n].w2, kD, kF), s));
      return 0;
    }
    return store_raw(e, "ssl." + k, src, shape, ndim, s);
  }
  // everything else on the path is a small fp32 tensor; off-path keys are dropped
  if (starts_with(k, "quantizer.") || starts_with(k, "project_q.") || starts_with(k, "final_proj.") ||
      k == "mask_emb" || starts_with(k, "target_glu") || starts_with(k, "layer_norm_") )
    return 0;
  return store_raw(e, "ssl." + k, src, shape, ndim, s);
}

static int load_conformer(afx_engine* e, const std::string& k, const float* src, const int64_t* shape, int ndim,
                          hipStream_t s) {
  const int E = e->E, Ep = e->Ep;
  if (k == "LL.weight") {
    if (expect_shape(k.c_str(), shape, ndim, {E, kD})) return 1;
    KOK(pack_linear(e, src, E, kD, kD, e->conf_ll, e->wscale(e->conf_ll, E, kD), s));
    return 0;
  }
  int b = 0;
  char tail[96];
  if (sscanf(k.c_str(), "conformer.encoder_blocks.%d.%95s", &b, tail) == 2) {
    if (b < 0 || b >= e->nblk) return fail("afx_load_weight: Conformer block %d out of range (n_encoders=%d)", b, e->nblk);
    ConfBlock& B = e->blk[b];
    const std::string t = tail;
    float* qkv_sc = e->wscale(B.wqkv, 3 * e->inner, Ep);
    struct { const char* name; void* dst; int N, K, Kp; float* sc; } lin[] = {
        {"ff1.fn.fn.net.0.weight", B.ff[0].w1, e->FF, E, Ep, e->wscale(B.ff[0].w1, e->FF, Ep)},
        {"ff1.fn.fn.net.3.weight", B.ff[0].w2, E, e->FF, e->FFp, e->wscale(B.ff[0].w2, E, e->FFp)},
        {"ff2.fn.fn.net.0.weight", B.ff[1].w1, e->FF, E, Ep, e->wscale(B.ff[1].w1, e->FF, Ep)},
        {"ff2.fn.fn.net.3.weight", B.ff[1].w2, E, e->FF, e->FFp, e->wscale(B.ff[1].w2, E, e->FFp)},
        {"attn.fn.to_q.weight", B.wqkv, e->inner, E, Ep, qkv_sc},
        {"attn.fn.to_kv.weight", (char*)B.wqkv + (size_t)e->inner * Ep * e->hsz, 2 * e->inner, E, Ep, qkv_sc ? qkv_sc + e->inner : nullptr},
        {"attn.fn.to_out.weight", B.wout, E, e->inner, Ep, e->wscale(B.wout, E, Ep)},
        {"conv.net.2.weight", B.pw1, 2 * e->C2, E, Ep, e->wscale(B.pw1, 2 * e->C2, Ep)},
        {"conv.net.7.weight", B.pw2, E, e->C2, e->C2p, e->wscale(B.pw2, E, e->C2p)},
    };
    for (auto& L : lin)
      if (t == L.name) {
        if (expect_shape(k.c_str(), shape, ndim, {L.N, L.K})) return 1;
        KOK(pack_linear(e, src, L.N, L.K, L.Kp, L.dst, L.sc, s));
        return 0;
      }
  }
  return store_raw(e, k, src, shape, ndim, s);
}

extern "C" int afx_load_weight(afx_handle h, const char* name, const float* dev_ptr, const int64_t* shape, int ndim,
                               void* stream) {
  if (!h || !name || !dev_ptr || (ndim > 0 && !shape)) return fail("afx_load_weight: null argument");
  hipStream_t s = (hipStream_t)stream;
  std::string k = name;
  if (starts_with(k, "module.")) k = k.substr(7);  // utils.py:13-43
  if (ends_with(k, "num_batches_tracked")) return 0;
  h->finalized = false;
  h->loaded.insert(k);
  if (starts_with(k, "ssl_model.model.")) return load_ssl(h, k.substr(16), dev_ptr, shape, ndim, s);
  if (h->cfg.arch == AFX_ARCH_SSL) {
    if (starts_with(k, "model.")) {
      h->loaded.insert("ssl_model." + k);
      return load_ssl(h, k.substr(6), dev_ptr, shape, ndim, s);
    }
    return 0;
  }
  if (h->cfg.arch == AFX_ARCH_CONFORMER_HEAD && (k == "LL.weight" || starts_with(k, "LL.") || starts_with(k, "first_bn."))) return 0;
  if (h->cfg.arch == AFX_ARCH_CONFORMER || h->cfg.arch == AFX_ARCH_CONFORMER_HEAD) return load_conformer(h, k, dev_ptr, shape, ndim, s);
  // AASIST head: everything is small fp32; bn1.* never influences the output (Q2)
  if (k.find(".bn1.") != std::string::npos) return 0;
  return store_raw(h, k, dev_ptr, shape, ndim, s);
}

// ---------------------------------------------------------------------------------
// resolve_weights: THE list of the tensors the launch paths read.  Run by every afx_finalize (afx_load_weight may have replaced
// any buffer since the last one), it checks each tensor for presence and for the element count the launches read, and stores
// the pointer in the tables of afx_engine.  A tensor a launch is to read is declared here and nowhere else; a null field after
// a successful finalize means "absent by mode" (set explicitly below), never a lookup that missed.
// ---------------------------------------------------------------------------------
struct LnRef { LnW* ln; int C; };
struct Resolver {
  afx_engine* e;
  const char *ckpt, *key;  // the prefix of the checkpoint's own names (what errors quote), and the one `f` keeps them under
  std::vector<LnRef>& lns;
  int missing(const std::string& k) const { return fail("afx_finalize: missing weight '%s%s'", ckpt, k.c_str()); }
  // a matrix packed into its operand form by afx_load_weight, which checked its shape
  int packed(const std::string& k) const { return e->loaded.count(ckpt + k) ? 0 : missing(k); }
  // a raw fp32 tensor of n elements (out null: only finalize itself reads it, by name)
  int raw(const std::string& k, size_t n, const float** out = nullptr) const {
    auto it = e->f.find(key + k);
    if (it == e->f.end()) return missing(k);
    if (it->second.n != n) return fail("afx_finalize: weight '%s%s' has %zu elements, expected %zu", ckpt, k.c_str(), it->second.n, n);
    if (out) *out = it->second.p;
    return 0;
  }
  int ln(const std::string& k, int C, LnW& w) const {
    w = LnW();
    if (raw(k + ".weight", C, &w.g) || raw(k + ".bias", C, &w.b)) return 1;
    lns.push_back({&w, C});
    return 0;
  }
};

static int resolve_weights(afx_engine* e, std::vector<LnRef>& lns) {
  const bool gn = e->cfg.extractor_mode == AFX_EXTRACTOR_GROUP_NORM;
  const bool head_only = e->cfg.arch == AFX_ARCH_CONFORMER_HEAD;
  if (!head_only) {
    const Resolver r{e, "ssl_model.model.", "ssl.", lns};
    for (int i = 0; i < 7; ++i) {
      const std::string c = "feature_extractor.conv_layers." + std::to_string(i);
      ConvLayer& L = e->conv[i] = ConvLayer();
      if (i == 0 ? r.raw(c + ".0.weight", (size_t)kC * kConvK[0], &L.w0) : r.packed(c + ".0.weight")) return 1;
      if (gn) {  // wav2vec2-base: bias-free convs, GroupNorm(512,512) on layer 0 only
        if (i == 0 && (r.raw(c + ".2.weight", kC, &L.gn_g) || r.raw(c + ".2.bias", kC, &L.gn_b))) return 1;
      } else if (r.raw(c + ".0.bias", kC, &L.bias) || r.ln(c + ".2.1", kC, L.ln)) {
        return 1;
      }
    }
    if (r.ln("layer_norm", kC, e->feat_ln) || r.packed("post_extract_proj.weight") || r.raw("post_extract_proj.bias", kD, &e->proj_b) ||
        r.raw("encoder.pos_conv.0.bias", kD, &e->pos_b) || r.ln("encoder.layer_norm", kD, e->enc_ln))
      return 1;
    for (int l = 0; l < e->cfg.n_layers; ++l) {
      const std::string P = "encoder.layers." + std::to_string(l) + ".";
      TrunkLayer& L = e->layers[l];
      for (const char* k : {"self_attn.q_proj.weight", "self_attn.q_proj.bias", "self_attn.k_proj.weight", "self_attn.k_proj.bias",
                            "self_attn.v_proj.weight", "self_attn.v_proj.bias", "self_attn.out_proj.weight", "fc1.weight", "fc2.weight"})
        if (r.packed(P + k)) return 1;
      if (r.raw(P + "self_attn.out_proj.bias", kD, &L.bo) || r.ln(P + "self_attn_layer_norm", kD, L.ln1) ||
          r.raw(P + "fc1.bias", kF, &L.b1) || r.raw(P + "fc2.bias", kD, &L.b2) || r.ln(P + "final_layer_norm", kD, L.ln2))
        return 1;
    }
  }
  if (e->cfg.arch == AFX_ARCH_CONFORMER || head_only) {
    const Resolver r{e, "", "", lns};
    const int E = e->E, C2 = e->C2;
    e->ll_b = nullptr;  // head only: MyConformer starts from its tokens, no LL / first_bn in the handle
    if (!head_only) {
      if (r.packed("LL.weight") || r.raw("LL.bias", E, &e->ll_b)) return 1;
      for (const char* k : {"first_bn.weight", "first_bn.bias", "first_bn.running_mean", "first_bn.running_var"})
        if (r.raw(k, 1)) return 1;
    }
    if (r.raw("conformer.class_token", E, &e->class_token) || r.raw("conformer.fc5.weight", (size_t)2 * E, &e->fc5_w) ||
        r.raw("conformer.fc5.bias", 2, &e->fc5_b))
      return 1;
    for (int b = 0; b < e->nblk; ++b) {
      const std::string P = "conformer.encoder_blocks." + std::to_string(b) + ".";
      ConfBlock& K = e->blk[b];
      for (int i = 0; i < 2; ++i) {
        const std::string ff = P + (i ? "ff2.fn." : "ff1.fn.");
        if (r.ln(ff + "norm", E, K.ff[i].ln) || r.packed(ff + "fn.net.0.weight") || r.raw(ff + "fn.net.0.bias", e->FF, &K.ff[i].b1) ||
            r.packed(ff + "fn.net.3.weight") || r.raw(ff + "fn.net.3.bias", E, &K.ff[i].b2))
          return 1;
      }
      if (r.ln(P + "attn.norm", E, K.attn_ln) || r.packed(P + "attn.fn.to_q.weight") || r.packed(P + "attn.fn.to_kv.weight") ||
          r.packed(P + "attn.fn.to_out.weight") || r.raw(P + "attn.fn.to_out.bias", E, &K.bout) ||
          r.raw(P + "attn.fn.rel_pos_emb.weight", (size_t)1025 * e->dh, &K.rel32) || r.ln(P + "conv.net.0", E, K.conv_ln) ||
          r.packed(P + "conv.net.2.weight") || r.raw(P + "conv.net.2.bias", (size_t)2 * C2, &K.bpw1) ||
          r.raw(P + "conv.net.4.conv.weight", (size_t)C2 * e->ck, &K.dw_w) || r.raw(P + "conv.net.4.conv.bias", C2, &K.dw_b))
        return 1;
      for (const char* k : {"conv.net.5.weight", "conv.net.5.bias", "conv.net.5.running_mean", "conv.net.5.running_var"})
        if (r.raw(P + k, C2)) return 1;  // (fold_bn)
      if (r.packed(P + "conv.net.7.weight") || r.raw(P + "conv.net.7.bias", E, &K.bpw2) || r.ln(P + "post_norm", E, K.post_ln)) return 1;
    }
  }
  return 0;
}

static int fold_bn(afx_engine* e, const std::string& p, int n, float* scale, float* shift, hipStream_t s) {
  const float *w = e->F(p + "weight"), *b = e->F(p + "bias"), *m = e->F(p + "running_mean"), *v = e->F(p + "running_var");
  if (!w || !b || !m || !v) return fail("afx_finalize: BatchNorm '%s*' incomplete", p.c_str());
  hipLaunchKernelGGL(bn_fold_kernel, dim3((n + 255) / 256), dim3(256), 0, s, w, b, m, v, kBnEps, n, scale, shift);
  HIP_OK(hipGetLastError());
  return 0;
}

// split precision: one scale per LayerNorm of the tables (LnW::scale) from the maxima of its gain and offset
static int s3_layernorm_scales(afx_engine* h, const std::vector<LnRef>& lns, hipStream_t s) {
  if (!h->s3 || lns.empty()) return 0;
  float* d = nullptr;
  HIP_OK(hipMalloc((void**)&d, lns.size() * 8));
  for (size_t i = 0; i < lns.size(); ++i) {
    hipLaunchKernelGGL(absmax_kernel, dim3(1), dim3(256), 0, s, lns[i].ln->g, lns[i].C, d + 2 * i);
    hipLaunchKernelGGL(absmax_kernel, dim3(1), dim3(256), 0, s, lns[i].ln->b, lns[i].C, d + 2 * i + 1);
  }
  std::vector<float> m(2 * lns.size());
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(m.data(), d, m.size() * 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  (void)hipFree(d);
  if (e != hipSuccess) return fail("afx_finalize: %s", hipGetErrorString(e));
  for (size_t i = 0; i < lns.size(); ++i) {
    const float bound = sqrtf((float)lns[i].C) * m[2 * i] + m[2 * i + 1];
    float sc = kS3ScaleBounded;
    while (sc * bound > 60000.f && sc > 1e-6f) sc *= 0.5f;  // (a non-finite gain stays non-finite: the overflow guard reports it)
    lns[i].ln->scale = sc;
  }
  return 0;
}

extern "C" int afx_finalize(afx_handle h, void* stream) {
  if (!h) return fail("afx_finalize: null handle");
  hipStream_t s = (hipStream_t)stream;
  const bool gn = h->cfg.extractor_mode == AFX_EXTRACTOR_GROUP_NORM;
  const bool head_only = h->cfg.arch == AFX_ARCH_CONFORMER_HEAD;
  std::vector<LnRef> lns;  // the LayerNorms of the tables
  if (resolve_weights(h, lns)) return 1;
  if (!head_only) {
    if (!gn && (h->dt != AFX_DT_FP32 || h->s3)) {  // conv layer 0 as the split-precision fp16 matrix-core operand
      if (!h->conv0pack && !(h->conv0pack = h->dalloc(conv0_pack_bytes()))) return fail("afx_finalize: device allocation failed");
      KOK(launch_conv0_pack(h->conv[0].w0, h->conv[0].bias, h->conv0pack, s));
    }
    // positional conv: weight-norm (dim=2) folded into the packed operand
    const float* pv = h->F("ssl.encoder.pos_conv.0.weight_v");
    const float* pg = h->F("ssl.encoder.pos_conv.0.weight_g");
    const float* pw = h->F("ssl.encoder.pos_conv.0.weight");
    if (pv && pg) {
      KOK(launch_pack_posconv(pv, pg, kD, kD / kPosG, kPosK, h->pos_norm, h->posw, h->dt, s));
    } else if (pw) {
      KOK(launch_pack_posconv(pw, nullptr, kD, kD / kPosG, kPosK, h->pos_norm, h->posw, h->dt, s));
    } else {
      return fail("afx_finalize: missing weight 'ssl_model.model.encoder.pos_conv.0.weight_g/weight_v'");
    }
    if (h->s3) KOK(launch_split_weight_rows(h->posw, kD, (kD / kPosG) * kPosK, h->wscale(h->posw, kD, (size_t)(kD / kPosG) * kPosK), s));
  }
  if (h->cfg.arch == AFX_ARCH_CONFORMER || head_only) {
    for (int b = 0; b < h->nblk; ++b) {
      ConfBlock& K = h->blk[b];
      if (fold_bn(h, "conformer.encoder_blocks." + std::to_string(b) + ".conv.net.5.", h->C2, K.bn_scale, K.bn_shift, s)) return 1;
      KOK(launch_pack_linear(K.rel32, 1025, h->dh, 64, K.rel_h, h->dt, s));
      if (h->E == 144) {  // parameter blocks of the fused chains (layout: ChainParamOffsets in afx_kernels.h)
        auto put = [&](int st, int off, const float* v, int n) -> int {
          HIP_OK(hipMemcpyAsync(K.chain_prm[st] + off, v, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
          return 0;
        };
        for (int st = 0; st < 3; ++st) HIP_OK(hipMemsetAsync(K.chain_prm[st], 0, (kChainParamFloats + kChainScaleFloats) * 4, s));
        for (int st = 0; st < 3; st += 2) {  // stages 0 and 2 carry a feed-forward module
          const ConfFF& ff = K.ff[st / 2];
          if (put(st, CP_FF_G, ff.ln.g, 144) || put(st, CP_FF_B, ff.ln.b, 144) || put(st, CP_FF_B1, ff.b1, 576) || put(st, CP_FF_B2, ff.b2, 144))
            return 1;
        }
        if (put(0, CP_LN2_G, K.attn_ln.g, 144) || put(0, CP_LN2_B, K.attn_ln.b, 144) ||
            put(1, CP_LN2_G, K.conv_ln.g, 144) || put(1, CP_LN2_B, K.conv_ln.b, 144) ||
            put(1, CP_BA, K.bout, 144) || put(1, CP_BB, K.bpw1, 576) ||
            put(2, CP_LN2_G, K.post_ln.g, 144) || put(2, CP_LN2_B, K.post_ln.b, 144) ||
            put(2, CP_BA, K.bpw2, 144))
          return 1;
        if (h->s3) {  // the weight rows' scales, per output column, behind the parameter block (ChainScaleOffsets)
          auto sc = [&](int st, int off, const void* w, int rows, int kp) -> int {
            HIP_OK(hipMemcpyAsync(K.chain_prm[st] + kChainParamFloats + off, h->wscale(w, rows, kp), (size_t)rows * 4, hipMemcpyDeviceToDevice, s));
            return 0;
          };
          if (sc(0, CS_FF1, K.ff[0].w1, h->FF, h->Ep) || sc(0, CS_FF2, K.ff[0].w2, h->E, h->FFp) || sc(0, CS_A, K.wqkv, 3 * h->inner, h->Ep) ||
              sc(1, CS_A, K.wout, h->E, h->Ep) || sc(1, CS_B, K.pw1, 2 * h->C2, h->Ep) ||
              sc(2, CS_A, K.pw2, h->E, h->C2p) || sc(2, CS_FF1, K.ff[1].w1, h->FF, h->Ep) || sc(2, CS_FF2, K.ff[1].w2, h->E, h->FFp))
            return 1;
        }
      }
    }
    if (head_only) {
      if (int rc = s3_layernorm_scales(h, lns, s)) return rc;
      h->finalized = true;
      return 0;
    }
    // BatchNorm2d(1): four scalars -> host (one-off synchronisation)
    float w, b, m, v;
    HIP_OK(hipStreamSynchronize(s));
    HIP_OK(hipMemcpy(&w, h->F("first_bn.weight"), 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(&b, h->F("first_bn.bias"), 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(&m, h->F("first_bn.running_mean"), 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(&v, h->F("first_bn.running_var"), 4, hipMemcpyDeviceToHost));
    h->conf_bn_scale = w / sqrtf(v + kBnEps);
    h->conf_bn_shift = b - m * h->conf_bn_scale;
  } else if (h->cfg.arch == AFX_ARCH_XLSR_AASIST) {
    h->aw.split = h->s3 || h->dt != AFX_DT_FP32;  // exact mode keeps the true-fp32 matrix instruction
    if (const char* m = aasist_finalize(
            h->aw, [&](const std::string& k) { return h->F(k); }, [&](size_t bytes) { return h->dalloc(bytes); }, s))
      return fail("afx_finalize: %s", m);
  }
  if (int rc = s3_layernorm_scales(h, lns, s)) return rc;
  h->finalized = true;
  return 0;
}

// ---------------------------------------------------------------------------------
// workspace carving (identical walk for sizing and for the real call)
// ---------------------------------------------------------------------------------
struct Carver {
  char* base;
  size_t off = 0, largest = 0;
  explicit Carver(void* b) : base((char*)b) {}
  void* take(size_t bytes) {
    if (bytes > largest) largest = bytes;
    off = (off + 255) & ~(size_t)255;
    void* p = base ? base + off : nullptr;
    off += bytes;
    return p;
  }
};

struct Ws {
  int T[7];
  void *bufA = nullptr, *bufB = nullptr, *feats_h = nullptr, *xpad = nullptr, *hbuf = nullptr, *qkv = nullptr, *att = nullptr, *ff = nullptr,
       *ssl_h = nullptr;
  float *tmp32 = nullptr, *x = nullptr, *ssl_f = nullptr;
  void* s3planes = nullptr;   // split precision: scratch for the pair form of the current product's A operand
  size_t s3bytes = 0;
  float* gn_stats = nullptr;  // group-norm extractor mode: partial sums + mean / rstd of conv layer 0
  // ragged batch (afx_forward_ragged): valid SSL frames per utterance on the device (null = uniform batch), and the
  // AASIST bucket buffers (utterances of equal length gathered into a uniform sub-batch for the graph back-end)
  int* lens = nullptr;
  float *bucket_f = nullptr, *bucket_logits = nullptr;
  // Conformer
  float *ll32 = nullptr, *xc = nullptr, *qkv32 = nullptr, *glu32 = nullptr;
  void *hc = nullptr, *hid = nullptr, *ao = nullptr, *u = nullptr;
  // AASIST
  AasistWs aa;
};

// Three entry shapes share one walk: the whole path (L > 0 samples), the path from the output of conv layer 5
// (T5 > 0 frames: afx_tail_forward, the streaming mode's per-hop call), the head alone (Tfeat SSL frames).
static size_t carve(const afx_engine* e, int B, int L, int Tfeat, void* base, Ws* w, int T5 = 0, bool ragged = false) {
  Carver c(base);
  const size_t hs = dtype_size(e->dt);
  int T = Tfeat;
  w->lens = nullptr;
  w->bucket_f = w->bucket_logits = nullptr;
  if (L > 0 || T5 > 0) {
    if (L > 0) {
      conv_lengths(L, w->T);
      const size_t n0 = (size_t)B * w->T[0] * kC, n1 = (size_t)B * w->T[1] * kC;
      w->bufA = c.take(n0 * hs);
      w->bufB = c.take(n1 * hs);
      w->tmp32 = (float*)c.take(n1 * 4);
      if (e->cfg.extractor_mode == AFX_EXTRACTOR_GROUP_NORM) w->gn_stats = (float*)c.take(conv0_groupnorm_stats_floats(B, w->T[0]) * 4);
    } else {
      for (int i = 0; i < 5; ++i) w->T[i] = 0;
      w->T[5] = T5;
      w->T[6] = T5 >= kConvK[6] ? (T5 - kConvK[6]) / kConvS[6] + 1 : 0;
      w->bufA = w->bufB = nullptr;
      w->tmp32 = (float*)c.take((size_t)B * (w->T[6] > 0 ? w->T[6] : 1) * kC * 4);
    }
    T = w->T[6];
    w->feats_h = c.take((size_t)B * T * kC * hs);
    w->x = (float*)c.take((size_t)B * T * kD * 4);
    w->xpad = c.take((size_t)B * (T + kPosK) * kD * hs);
    w->hbuf = c.take((size_t)B * T * kD * hs);
    w->qkv = c.take((size_t)B * T * 3 * kD * hs);
    w->att = c.take((size_t)B * T * kD * hs);
    w->ff = c.take((size_t)B * T * kF * hs);
  }
  w->ssl_f = (float*)c.take((size_t)B * T * kD * 4);
  w->ssl_h = c.take((size_t)B * T * kD * hs);
  if (ragged) {
    w->lens = (int*)c.take((size_t)B * 4);
    if (e->cfg.arch == AFX_ARCH_XLSR_AASIST) {
      w->bucket_f = (float*)c.take((size_t)B * T * kD * 4);
      w->bucket_logits = (float*)c.take((size_t)B * 2 * 4);
    }
  }
  if (e->cfg.arch == AFX_ARCH_CONFORMER || e->cfg.arch == AFX_ARCH_CONFORMER_HEAD) {
    const size_t M = (size_t)B * (T + 1);
    w->ll32 = (float*)c.take((size_t)B * T * e->E * 4);
    w->xc = (float*)c.take(M * e->E * 4);
    w->qkv32 = (float*)c.take(M * 3 * e->inner * 4);
    w->glu32 = (float*)c.take(M * 2 * e->C2 * 4);
    w->hc = c.take(M * e->Ep * hs);
    w->hid = c.take(M * e->FFp * hs);
    w->ao = c.take(M * e->Ep * hs);
    w->u = c.take(M * e->C2p * hs);
  } else if (e->cfg.arch == AFX_ARCH_XLSR_AASIST) {
    aasist_carve(B, T, [&](size_t bytes) { return c.take(bytes); }, &w->aa);
  }
  w->s3planes = nullptr;
  w->s3bytes = 0;
  if (e->s3) {  // two fp16 planes of the largest operand = the bytes of its fp32 form (+ the plane alignment)
    size_t big = c.largest;
    if (T5 > 0 && (size_t)B * T5 * kC * 4 > big) big = (size_t)B * T5 * kC * 4;  // (tail mode: the caller's layer-5 frames)
    w->s3bytes = big + 4096;
    w->s3planes = c.take(w->s3bytes);
  }
  return c.off + 256;
}

extern "C" int afx_num_frames(int n) {
  int T[7];
  conv_lengths(n, T);
  return T[6];
}

extern "C" size_t afx_workspace_bytes(afx_handle h, int B, int L) {
  if (!h || B <= 0 || L <= 0) return 0;
  Ws w;
  return carve(h, B, L, 0, nullptr, &w);
}

// ---------------------------------------------------------------------------------
// taps (debug): engine-owned fp32 copies of intermediates
// ---------------------------------------------------------------------------------
__global__ void half_to_f32_kernel(const uint16_t* in, float* out, size_t n, int is_bf16) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    if (is_bf16) {
      out[i] = __uint_as_float((unsigned)in[i] << 16);
    } else {
      _Float16 hv;
      memcpy(&hv, &in[i], 2);
      out[i] = (float)hv;
    }
  }
}
// split precision: a buffer of pair-form rows (row stride ld fp32 elements) -> the fp32 values its consumer reads,
// (hi + lo) / scale per element (afx_kernels.h::s3_pair_index), in the buffer's own row layout
__global__ void pairs_to_f32_kernel(const uint16_t* in, float* out, size_t n, long ld, float inv_scale) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t r = i / ld;
    const long k = (long)(i - r * ld);
    const uint16_t* row = in + r * 2 * ld;
    _Float16 hi, lo;
    memcpy(&hi, &row[s3_pair_index(k)], 2);
    memcpy(&lo, &row[s3_pair_index(k) + 32], 2);
    out[i] = ((float)hi + (float)lo) * inv_scale;
  }
}
extern "C" int afx_tap(afx_handle h, const char* name, float* out, size_t cap, size_t* n_out, void* stream) {
  if (!h || !name) return fail("afx_tap: null argument");
  auto it = h->taps.find(name);
  if (it == h->taps.end()) return fail("afx_tap: no tap named '%s' (enable taps and run a forward first)", name);
  if (n_out) *n_out = it->second.n;
  if (out) {
    if (cap < it->second.n) return fail("afx_tap: buffer too small (%zu < %zu)", cap, it->second.n);
    HIP_OK(hipMemcpyAsync(out, it->second.p, it->second.n * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  }
  return 0;
}

// ---------------------------------------------------------------------------------
// per-kernel-class timing (bench.py's roofline leg): when profiling is on, every
// launch of the forward is bracketed by hipEvents on the launch stream and summed per
// class afterwards.  Off by default: the normal forward records nothing.
// ---------------------------------------------------------------------------------
enum ProfClass { PC_GEMM128 = 0, PC_GEMM64, PC_GEMM64_DEEP, PC_GEMM256, PC_GEMM_ROWLN, PC_GEMM8_256, PC_GEMM8_ROWLN, PC_GEMM_F32, PC_CONV0, PC_POSCONV, PC_ROWNORM, PC_MHSA, PC_CONF_ATTN, PC_CONF_DWCONV, PC_CONF_CHAIN,
                 PC_MISC, PC_AASIST, PC_COUNT };
static const char* kProfNames[PC_COUNT] = {"gemm_kernel<128x128>", "gemm_kernel<128x64>", "gemm_deep_kernel<128x64>", "gemm_kernel<256x256>",
                                           "gemm_kernel<128x512,rowLN>", "gemm8_kernel<256x256>", "gemm8_kernel<128x512,rowLN>", "gemm_f32_kernel<128x128>", "conv0_kernel", "posconv_kernel", "rownorm_kernel", "mhsa_kernel", "conf_attn_kernel",
                                           "conf_dwconv_kernel", "conf_chain_kernel", "misc", "aasist_head"};
struct ProfRec { int cls; hipEvent_t a, b; double flops; };
struct Profiler {
  bool on = false;
  std::vector<ProfRec> recs;
  std::vector<hipEvent_t> pool;
  size_t used = 0;
  hipEvent_t ev() {
    if (used == pool.size()) {
      hipEvent_t e;
      if (hipEventCreate(&e) != hipSuccess) return nullptr;
      pool.push_back(e);
    }
    return pool[used++];
  }
};
static void prof_forget(afx_engine* e) {
  if (!e->prof) return;
  for (hipEvent_t ev : e->prof->pool) (void)hipEventDestroy(ev);
  delete e->prof;
  e->prof = nullptr;
}

// ---------------------------------------------------------------------------------
// The call context: ONE native call on ONE handle.  Every entry point that launches builds a Call on its stack and hands it
// by reference to whatever launches for it; nothing here is shared between calls, handles or threads, and nothing of it
// outlives the call except the handle's `last_objective` read-back.  It holds the stream, the launch-shape objective (read
// once from the handle's "concurrent" switch: fixed for the whole call), the handle's profiler, and -- split precision -- the
// pair-form scratch of the workspace the call runs in with the registry below.  The engine's other switches ("gemm_small_deep")
// and its weight tables are read from `e` where they are used.
// Pair-form registry: operand buffers whose ONLY readers are dense products may receive their producer's result directly as
// the product's A operand (the PAIR FORM of the row -- afx_kernels.h -- in place of its fp32 values: same bytes, row by row) --
// the LayerNorms, the GELU / LayerNorm epilogues of the products and the attention write the operand themselves and the
// separate split launch disappears.  s3ok: the buffers of this call that qualify; s3reg: which of them currently hold
// pair-form rows.
// ---------------------------------------------------------------------------------
constexpr int kS3Bufs = 10;
struct S3Reg { const void* p; float scale; };  // scale: the power of two the rows were multiplied by before the split (0: fp32 values)
struct Call {
  afx_engine* const e;
  const hipStream_t s;
  const int objective;   // OBJ_*: every product and chain of the call is shaped for it (GemmArgs / ConfChainArgs::objective)
  Profiler* const prof;
  void* const s3planes;  // null: not a split-precision engine
  const size_t s3bytes;
  const void* s3ok[kS3Bufs] = {nullptr};
  S3Reg s3reg[kS3Bufs] = {};

  Call(afx_engine* e_, void* stream, void* planes = nullptr, size_t bytes = 0, std::initializer_list<const void*> ok = {})
      : e(e_), s((hipStream_t)stream), objective(e_->concurrent ? OBJ_CU_TIME : OBJ_MAKESPAN), prof(e_->prof), s3planes(planes), s3bytes(bytes) {
    e->last_objective = dispatch_objective(objective);
    int i = 0;
    for (const void* p : ok)
      if (p && i < kS3Bufs) s3ok[i++] = p;
  }
  Call(afx_engine* e_, void* stream, const Ws& w)
      : Call(e_, stream, w.s3planes, w.s3bytes, {w.bufA, w.bufB, w.feats_h, w.hbuf, w.att, w.ff, w.xpad, w.hc, w.ssl_h, w.hid}) {}
  Call(const Call&) = delete;

  bool s3_ok(const void* p) const {
    if (!p || !s3planes) return false;
    for (const void* q : s3ok) if (q == p) return true;
    return false;
  }
  void s3_set(const void* p, float scale) {  // 0: the buffer holds fp32 values again
    for (S3Reg& r : s3reg) if (r.p == p) { r.scale = scale; if (scale == 0.f) r.p = nullptr; return; }
    if (scale == 0.f) return;
    for (S3Reg& r : s3reg) if (!r.p) { r = S3Reg{p, scale}; return; }
  }
  float s3_pairs_in(const void* p) const {  // the scale of the pair-form rows `p` holds, 0 when it holds fp32 values
    for (const S3Reg& r : s3reg) if (r.p && r.p == p) return r.scale;
    return 0.f;
  }
  template <class F>
  const char* timed(int cls, double flops, F&& f) {
    if (!prof || !prof->on) return f();
    hipEvent_t a = prof->ev(), b = prof->ev();
    if (!a || !b) return "profiler: hipEventCreate failed";
    (void)hipEventRecord(a, s);
    const char* m = f();
    (void)hipEventRecord(b, s);
    prof->recs.push_back({cls, a, b, flops});
    return m;
  }
  const char* gemm(const GemmArgs& g_in, int dt, int groups, bool rows = false);
  const char* rownorm(const RowNormArgs& a_in, const LnW& ln, int dt);
};
// Split precision (Call::gemm): x.w ~ xh.wl + xl.wh + xh.wh on the fp16 matrix pipe.  Both operands go in PAIR FORM
// (afx_kernels.h): the weight is stored that way with per-row scales behind it (pack_linear), the fp32 A operand is either
// already there (its producer wrote pair-form rows in place: s3_pairs_in) or the span the product addresses is converted into
// the workspace's scratch; ONE launch then walks the 2 K halfs of a row like a plain fp16 operand and issues three matrix
// instructions per K-step on the fragments it reads anyway (round 3 walked K three times over separate hi / lo planes: 1.5x
// the K-tiles, operand bytes and fragment reads for the same matrix-pipe work).
// rows: the product goes to launch_gemm_rows (GemmArgs::oh_rows holds its output row table)
const char* Call::gemm(const GemmArgs& g_in, int dt, int groups, bool rows) {
  GemmArgs g = g_in;
  g.no_deep = e->gemm_small_deep ? 0 : 1;
  g.objective = objective;
  const double fl = 2.0 * g.M * g.N * (g.k_algo ? g.k_algo : g.K) * groups;
  // profiler class of a tile id (afx_gemm.hip::gemm_tile_of): 92 = the deep form of the 128x64 tile, a class of its own
  auto cls_of = [](int tile) -> int {
    static const int cls[9] = {PC_GEMM128, PC_GEMM64, PC_GEMM256, PC_GEMM_ROWLN, PC_GEMM256, PC_GEMM256, PC_GEMM_ROWLN, PC_GEMM8_256, PC_GEMM8_ROWLN};
    return tile == 92 ? PC_GEMM64_DEEP : (tile >= 0 && tile < 9 ? cls[tile] : PC_GEMM128);
  };
  if (dt == DT_FP32 && s3planes) {
    const bool groups32 = !(g.K % 32 || g.kchunk % 32 || g.a_row % 32 || g.a_batch % 32 || g.g_a % 32 || g.kchunk_stride % 32 || g.ldw % 32 || g.g_w % 32);
    if (!groups32 || ((size_t)g.A & 15)) {  // (rows the pair form cannot address in whole 32-element groups: the fp32 instruction)
      if (rows) return "split-precision product with a row table: the operands must be pair-form addressable";
      if (g.out_h) s3_set(g.out_h, 0.f);
      return launch_gemm(g, DT_FP32, groups, s);
    }
    GemmArgs q = g;
    float a_scale = s3_pairs_in(g.A);
    if (a_scale == 0.f) {  // convert the span of A this product addresses (fp32 elements from g.A on) into the scratch
      const long last = g.M - 1;
      long span = (last / g.rpb) * g.a_batch + (last % g.rpb) * g.a_row + (long)(g.K / g.kchunk - 1) * g.kchunk_stride + g.kchunk +
                  (long)(groups - 1) * g.g_a;
      span = (span + 31) & ~31L;
      if ((size_t)span * 4 > s3bytes) return "split-precision product: the A operand exceeds the pair-form scratch";
      a_scale = kS3ScaleFree;
      if (const char* m = timed(PC_MISC, 0, [&] { return launch_split_pairs((const float*)g.A, span, s3planes, a_scale, s); })) return m;
      q.A = s3planes;
    }
    // every K-side length counts halfs of the pair form: twice the fp32-element value
    q.k1 = g.K;
    q.K = 2 * g.K;
    if (!q.k_algo) q.k_algo = g.K;
    q.kchunk = 2 * g.kchunk;
    q.kchunk_stride = 2 * g.kchunk_stride;
    q.a_row = 2 * g.a_row;
    q.a_batch = 2 * g.a_batch;
    q.g_a = 2 * g.g_a;
    q.ldw = 2 * g.ldw;
    q.g_w = 2 * g.g_w;
    q.pre_scale = (const float*)((const char*)g.W + (size_t)groups * g.N * g.ldw * 4);  // afx_engine::wscale
    q.a_inv = 1.0f / a_scale;
    // the result as the NEXT product's A operand, where only products read the buffer (pair-form rows in place of fp32 rows);
    // a LayerNorm epilogue bounds its output (the larger scale), anything else is unbounded in a trained checkpoint
    if (g.out_h) {
      const bool pairs_out = s3_ok(g.out_h) && (g.N & 7) == 0 && (g.g_n & 7) == 0 && (g.ldo_h & 31) == 0 && g.out_h != g.A;
      q.oh_pairs = pairs_out ? 1 : 0;
      q.oh_scale = g.ln_gamma ? kS3ScaleBounded : kS3ScaleFree;
      s3_set(g.out_h, pairs_out ? q.oh_scale : 0.f);
    }
    const int tile = gemm_tile_of(q, groups);
    return timed(cls_of(tile), fl, [&] { return rows ? launch_gemm_rows(q, DT_FP16X3, s) : launch_gemm(q, DT_FP16X3, groups, s); });
  }
  if (rows && (dt == DT_FP32 || groups != 1)) return "gemm with a row table: half- or split-precision operands, one group";
  return timed(dt == DT_FP32 ? PC_GEMM_F32 : cls_of(gemm_tile_of(g, groups)), fl,
               [&] { return rows ? launch_gemm_rows(g, dt, s) : launch_gemm(g, dt, groups, s); });
}
// the rows of `a_in` (plain_norm) through the LayerNorm `ln` of the weight tables
const char* Call::rownorm(const RowNormArgs& a_in, const LnW& ln, int dt) {
  RowNormArgs a = a_in;
  a.gamma = ln.g; a.beta = ln.b;
  if (a.out_h && s3planes) {  // split precision: the LayerNorm writes the next product's A operand (pair-form rows) itself
    const bool pairs_out = dt == DT_FP32 && s3_ok(a.out_h) && (a.ldo_h & 31) == 0 && a.out_h != (const void*)a.x;
    a.oh_pairs = pairs_out ? 1 : 0;
    a.oh_scale = ln.scale;  // |LayerNorm output| <= sqrt(C) max|gamma| + max|beta|: the scale finalize chose for this LayerNorm
    s3_set(a.out_h, pairs_out ? a.oh_scale : 0.f);
  }
  return timed(PC_ROWNORM, 0, [&] { return launch_rownorm(a, dt, s); });
}

// debug tap: an engine-owned fp32 copy of an intermediate (afx_tap reads it back)
// is_half: `src` is an operand buffer (operand type; split precision: fp32 rows or pair-form rows of stride ld elements)
static int tap(Call& cx, const char* name, const void* src, size_t n, bool is_half, long ld = 0) {
  afx_engine* e = cx.e;
  if (!e->taps_on) return 0;
  TapRec& t = e->taps[name];
  if (t.cap < n) {
    if (t.p) (void)hipFree(t.p);
    HIP_OK(hipMalloc((void**)&t.p, n * 4));
    t.cap = n;
  }
  t.n = n;
  const float pair_scale = is_half && e->s3 ? cx.s3_pairs_in(src) : 0.f;
  if (pair_scale != 0.f) {
    if (ld <= 0 || ld % 32 || n % ld) return fail("tap '%s': pair-form rows need a row stride that is a multiple of 32", name);
    hipLaunchKernelGGL(pairs_to_f32_kernel, dim3(1024), dim3(256), 0, cx.s, (const uint16_t*)src, t.p, n, ld, 1.0f / pair_scale);
    HIP_OK(hipGetLastError());
  } else if (is_half && e->dt != AFX_DT_FP32) {
    hipLaunchKernelGGL(half_to_f32_kernel, dim3(1024), dim3(256), 0, cx.s, (const uint16_t*)src, t.p, n,
                       e->dt == AFX_DT_BF16 ? 1 : 0);
    HIP_OK(hipGetLastError());
  } else {
    HIP_OK(hipMemcpyAsync(t.p, src, n * 4, hipMemcpyDeviceToDevice, cx.s));
  }
  return 0;
}

extern "C" int afx_profile_begin(afx_handle h) {
  if (!h) return fail("afx_profile_begin: null handle");
  if (!h->prof) h->prof = new Profiler();
  Profiler& p = *h->prof;
  p.on = true;
  p.recs.clear();
  p.used = 0;
  return 0;
}
extern "C" int afx_profile_end(afx_handle h, int n, double* ms, double* flops, long long* launches) {
  if (!h || n < PC_COUNT || !ms || !flops || !launches) return fail("afx_profile_end: need %d slots", (int)PC_COUNT);
  if (!h->prof) return fail("afx_profile_end: afx_profile_begin was not called on this handle");
  Profiler& p = *h->prof;
  for (int i = 0; i < n; ++i) { ms[i] = 0; flops[i] = 0; launches[i] = 0; }
  for (const ProfRec& r : p.recs) {
    HIP_OK(hipEventSynchronize(r.b));
    float t = 0;
    HIP_OK(hipEventElapsedTime(&t, r.a, r.b));
    ms[r.cls] += t;
    flops[r.cls] += r.flops;
    launches[r.cls] += 1;
  }
  p.on = false;
  p.recs.clear();
  p.used = 0;
  return 0;
}
extern "C" int afx_profile_num_classes(void) { return PC_COUNT; }
extern "C" const char* afx_profile_class_name(int c) { return c >= 0 && c < PC_COUNT ? kProfNames[c] : ""; }

// ---------------------------------------------------------------------------------
// forward pieces
// ---------------------------------------------------------------------------------
static GemmArgs plain_gemm(const void* A, long lda, const void* W, long ldw, int M, int N, int K) {
  GemmArgs g;
  memset(&g, 0, sizeof g);
  g.A = A; g.W = W; g.M = M; g.N = N; g.K = K;
  g.rpb = M; g.a_batch = 0; g.a_row = lda;
  g.kchunk = K; g.kchunk_stride = 0; g.ldw = ldw;
  g.alpha = 1.f; g.act = ACT_NONE;
  g.o_batch_rows = M; g.oh_batch_rows = M;
  return g;
}

static RowNormArgs plain_norm(const float* x, long ldx, int rows, int C) {  // (gamma, beta: Call::rownorm)
  RowNormArgs a;
  memset(&a, 0, sizeof a);
  a.x = x; a.ldx = ldx; a.rows = rows; a.C = C; a.eps = kLnEps; a.act = ACT_NONE;
  a.rpb = rows; a.o_batch_rows = rows;
  return a;
}

// debug tap at a launch boundary (the name is only built while taps are on): op = an operand buffer of row stride ld
#define TAP(nm, p, n, op, ld)                                                                \
  do {                                                                                       \
    if (cx.e->taps_on && tap(cx, std::string(nm).c_str(), (p), (n), (op), (ld))) return 1; \
  } while (0)

// the positional conv as a grouped product (chunked K over time-padded operand rows) + GELU, added to x in place: `rows` =
// the first operand row of utterance 0's output frame 0, `batch_rows` operand rows from one utterance to the next, B x T frames
static const char* posconv_product(Call& cx, const void* rows, long batch_rows, int B, int T, float* x, int dt) {
  afx_engine* e = cx.e;
  const int cpg = kD / kPosG;
  GemmArgs g = plain_gemm(rows, 0, e->posw, (long)cpg * kPosK, B * T, cpg, cpg * kPosK);
  g.rpb = T; g.a_batch = batch_rows * kD; g.a_row = kD;
  g.kchunk = cpg; g.kchunk_stride = kD;
  g.g_a = cpg; g.g_w = (long)cpg * cpg * kPosK; g.g_n = cpg;
  g.bias = e->pos_b;
  g.act = ACT_GELU;
  g.resid = x; g.ldr = kD;
  g.out_f = x; g.ldo_f = kD; g.o_batch_rows = T; g.oh_batch_rows = T;
  return cx.gemm(g, dt, kPosG);
}

// l5: null = start from the waveform; else the output of conv layer 5, (B, T[5], 512) operand type (tail mode)
// l5_batch: elements between two utterances of l5 (0 = packed, T[5] * 512): a streaming caller keeps its window inside a longer ring
static int run_trunk(Call& cx, const float* wave, int B, int L, Ws& w, const void* l5 = nullptr, long l5_batch = 0) {
  afx_engine* e = cx.e;
  const hipStream_t s = cx.s;
  const int dt = e->dt;
  const int* T = w.T;
  if (T[6] < 1) return fail("afx_forward: %d samples are too few for one output frame (need >= 400)", L);
  const ConvLayer& c0 = e->conv[0];
  // layer 0: waveform -> (B,T0,512) operand type, normalisation + GELU fused
  const bool gn = e->cfg.extractor_mode == AFX_EXTRACTOR_GROUP_NORM;
  if (!l5)
    KOK(cx.timed(PC_CONV0, 2.0 * B * T[0] * kC * kConvK[0], [&] {
      if (gn)  // wav2vec2-base: GroupNorm over time per (utterance, channel), two passes over the cheap convolution
        return launch_conv0_groupnorm(wave, B, L, T[0], c0.w0, c0.gn_g, c0.gn_b, kLnEps,
                                      w.gn_stats, w.bufA, dt, s);
      if (e->s3) {  // split precision: the same matrix-core kernel as the fp16 engines; its rows leave as conv layer 1's pair-form operand
        // (LayerNorm + GELU output: bounded by the LayerNorm's gains -- the scale finalize chose for it)
        const float sc = cx.s3_ok(w.bufA) ? c0.ln.scale : 0.f;
        cx.s3_set(w.bufA, sc);
        return launch_conv0(wave, B, L, T[0], c0.w0, c0.bias, c0.ln.g, c0.ln.b, e->cfg.pre_emphasis, e->cfg.pre_emphasis_coef, w.bufA, DT_FP16X3, s, e->conv0pack, sc);
      }
      return launch_conv0(wave, B, L, T[0], c0.w0, c0.bias, c0.ln.g, c0.ln.b, e->cfg.pre_emphasis, e->cfg.pre_emphasis_coef, w.bufA, dt, s,
                          e->conv0pack);
    }));
  if (!l5) TAP("c0", w.bufA, (size_t)B * T[0] * kC, true, kC);
  // layers 1..6: conv-as-GEMM on a row-complete tile, LayerNorm(512) + GELU fused into the
  // epilogue (the pre-norm fp32 activations never leave the registers)
  void* in = l5 ? const_cast<void*>(l5) : w.bufA;
  void* out = w.bufB;
  for (int i = l5 ? 6 : 1; i < 7; ++i) {
    const int M = B * T[i], K = kConvK[i] * kC;
    GemmArgs g = plain_gemm(in, 0, e->convw[i], K, M, kC, K);
    g.rpb = T[i]; g.a_batch = (l5 && i == 6 && l5_batch) ? l5_batch : (long)T[i - 1] * kC; g.a_row = (long)kConvS[i] * kC;
    g.o_batch_rows = T[i]; g.oh_batch_rows = T[i];
    g.bias = e->conv[i].bias;  // (group-norm mode: null)
    g.act = ACT_GELU;
    if (gn) {  // wav2vec2-base: conv -> GELU, nothing to normalise in layers 1-6 (plain product, GELU epilogue)
      if (i < 6) {
        g.out_h = out; g.ldo_h = kC;
      } else {
        g.out_f = w.tmp32; g.ldo_f = kC;
      }
      KOK(cx.gemm(g, dt, 1));
    } else if (e->fuse_conv_ln && dt != DT_FP32) {
      // (split precision takes the two-kernel form below: measured, the row-complete tile with the pair-form walk and the fp32
      // erf-GELU in its epilogue is SLOWER than the 256-wide tile + a LayerNorm pass that writes the next layer's pair-form
      // operand -- student 12.9 against 12.3 ms per forward, teacher 9.0 / 8.75: profiles/r04_s3_knobs.txt)
      g.ln_gamma = e->conv[i].ln.g; g.ln_beta = e->conv[i].ln.b; g.ln_eps = kLnEps;
      if (i < 6) {
        g.out_h = out; g.ldo_h = kC;
      } else {
        g.out_f = w.tmp32; g.ldo_f = kC;  // fp32: the feature LayerNorm follows
      }
      KOK(cx.gemm(g, dt, 1));
    } else {  // two-kernel form (kept for A/B measurements)
      g.act = ACT_NONE;
      g.out_f = w.tmp32; g.ldo_f = kC;
      KOK(cx.gemm(g, dt, 1));
      RowNormArgs n = plain_norm(w.tmp32, kC, M, kC);
      n.act = ACT_GELU;
      if (i < 6) {
        n.out_h = out; n.ldo_h = kC;
      } else {
        n.out_f = w.tmp32; n.ldo_f = kC;  // in place: a row is register-resident before it is written
      }
      KOK(cx.rownorm(n, e->conv[i].ln, dt));
    }
    if (i < 6) TAP("c" + std::to_string(i), out, (size_t)M * kC, true, kC);
    void* t = in; in = out; out = t;
  }
  const int Tt = T[6], M = B * Tt;
  if (tap(cx, "conv", w.tmp32, (size_t)M * kC, false)) return 1;
  // feature LayerNorm(512) -> operand type
  {
    RowNormArgs n = plain_norm(w.tmp32, kC, M, kC);
    n.out_h = w.feats_h; n.ldo_h = kC;
    KOK(cx.rownorm(n, e->feat_ln, dt));
  }
  TAP("feats", w.feats_h, (size_t)M * kC, true, kC);
  // post_extract_proj: fp32 residual stream x + operand copy into the time-padded buffer
  {
    GemmArgs g = plain_gemm(w.feats_h, kC, e->projw, kC, M, kD, kC);
    g.rpb = Tt; g.a_batch = (long)Tt * kC; g.a_row = kC;
    g.bias = e->proj_b;
    g.out_f = w.x; g.ldo_f = kD; g.o_batch_rows = Tt; g.o_row_off = 0;
    g.out_h = w.xpad; g.ldo_h = kD; g.oh_batch_rows = Tt + kPosK; g.oh_row_off = kPosPad;
    KOK(cx.gemm(g, dt, 1));
    // (ragged batch: the frames past an utterance's own length are zeroed too -- alone, its positional conv would
    // see zero padding there)
    KOK(cx.timed(PC_MISC, 0, [&] { return launch_zero_pad_rows(w.xpad, B, Tt, kD, kPosPad, kPosK - kPosPad, dt, s, w.lens); }));
  }
  TAP("xpad", w.xpad, (size_t)B * (Tt + kPosK) * kD, true, kD);
  if (tap(cx, "proj", w.x, (size_t)M * kD, false)) return 1;
  // positional conv (grouped, k=128) + GELU, added to x in place
  if (e->posconv_sliding && dt != DT_FP32 && Tt <= 224) {  // (reads the zero-padded operand copy: ragged batches need nothing more)
    PosConvArgs pc;
    memset(&pc, 0, sizeof pc);
    pc.xpad = w.xpad; pc.xpad_batch = (long)(Tt + kPosK) * kD; pc.W = e->posw; pc.bias = e->pos_b;
    pc.x = w.x; pc.B = B; pc.T = Tt;
    KOK(cx.timed(PC_POSCONV, 2.0 * M * kD * (kD / kPosG) * kPosK, [&] { return launch_posconv(pc, dt, s); }));
  } else {
    KOK(posconv_product(cx, w.xpad, Tt + kPosK, B, Tt, w.x, dt));
  }
  if (tap(cx, "pos", w.x, (size_t)M * kD, false)) return 1;
  // transformer layers (pre-LN)
  auto resid_product = [&](const void* A, long lda, const void* W, int K, const float* bias) -> const char* {
    GemmArgs o = plain_gemm(A, lda, W, K, M, kD, K);
    o.bias = bias; o.resid = w.x; o.ldr = kD; o.out_f = w.x; o.ldo_f = kD;
    return cx.gemm(o, dt, 1);
  };
  for (int l = 0; l < e->cfg.n_layers; ++l) {
    const TrunkLayer& L = e->layers[l];
    RowNormArgs n1 = plain_norm(w.x, kD, M, kD);
    n1.out_h = w.hbuf; n1.ldo_h = kD;
    KOK(cx.rownorm(n1, L.ln1, dt));
    auto lp = [l](const char* leaf) { return "l" + std::to_string(l) + "." + leaf; };  // (tap names: built only while taps are on)
    TAP(lp("ln1"), w.hbuf, (size_t)M * kD, true, kD);
    GemmArgs q = plain_gemm(w.hbuf, kD, L.wqkv, kD, M, 3 * kD, kD);
    q.bias = L.bqkv;
    q.out_h = w.qkv; q.ldo_h = 3 * kD;
    KOK(cx.gemm(q, dt, 1));
    TAP(lp("qkv"), w.qkv, (size_t)M * 3 * kD, true, 3 * kD);
    KOK(cx.timed(PC_MHSA, 4.0 * B * kH * (double)Tt * Tt * 64, [&] {
      if (e->s3 && Tt <= 224) {  // split precision: the matrix-core form; its output goes out as the output projection's A planes
        const bool pairs = cx.s3_ok(w.att);
        cx.s3_set(w.att, pairs ? kS3ScaleFree : 0.f);
        return launch_mhsa_split((const float*)w.qkv, (float*)w.att, B, Tt, kH, s, w.lens, pairs, kS3ScaleFree);
      }
      if (e->s3) cx.s3_set(w.att, 0.f);
      return launch_mhsa(w.qkv, w.att, B, Tt, kH, dt, s, w.lens);
    }));
    TAP(lp("att"), w.att, (size_t)M * kD, true, kD);
    KOK(resid_product(w.att, kD, L.wo, kD, L.bo));
    TAP(lp("mid"), w.x, (size_t)M * kD, false, kD);
    RowNormArgs n2 = plain_norm(w.x, kD, M, kD);
    n2.out_h = w.hbuf; n2.ldo_h = kD;
    KOK(cx.rownorm(n2, L.ln2, dt));
    TAP(lp("ln2"), w.hbuf, (size_t)M * kD, true, kD);
    GemmArgs f1 = plain_gemm(w.hbuf, kD, L.w1, kD, M, kF, kD);
    f1.bias = L.b1; f1.act = ACT_GELU;
    f1.out_h = w.ff; f1.ldo_h = kF;
    KOK(cx.gemm(f1, dt, 1));
    TAP(lp("ff"), w.ff, (size_t)M * kF, true, kF);
    KOK(resid_product(w.ff, kF, L.w2, kF, L.b2));
    if (e->taps_on) {
      const std::string nm = "layer" + std::to_string(l);
      if (tap(cx, nm.c_str(), w.x, (size_t)M * kD, false)) return 1;
    }
  }
  // final encoder LayerNorm -> fp32 features (API output / AASIST input) + operand copy (LL GEMM)
  RowNormArgs nf = plain_norm(w.x, kD, M, kD);
  nf.out_f = w.ssl_f; nf.ldo_f = kD;
  nf.out_h = w.ssl_h; nf.ldo_h = kD;
  nf.nonfinite = e->nonfinite;  // overflow guard: an operand copy that left fp16's range anywhere in the trunk ends here as inf / NaN
  nf.nf_lens = w.lens; nf.nf_rpb = Tt;  // (ragged batch: only the rows of an utterance's own length are judged; the others hold stale workspace)
  KOK(cx.rownorm(nf, e->enc_ln, dt));
  if (tap(cx, "ssl", w.ssl_f, (size_t)M * kD, false)) return 1;
  TAP("ssl.op", w.ssl_h, (size_t)M * kD, true, kD);
  return 0;
}

// Conformer head from SSL features already in w.ssl_h (operand type)
// tokens: null = from the SSL features in w.ssl_h (Model / MyModel.forward); else the (B,T,E) fp32 rows MyConformer.forward
// is given (models/conformer_baseline.py:22-29).  embedding (device (B,E) fp32, may be null) receives token 0 of every utterance.
static int run_conformer(Call& cx, int B, int T, Ws& w, float* logits, const float* tokens = nullptr, float* embedding = nullptr) {
  afx_engine* e = cx.e;
  const hipStream_t s = cx.s;
  const int dt = e->dt, E = e->E, Ep = e->Ep, N = T + 1, M = B * N;
  if (tokens) {  // class token + the rows as they are
    KOK(cx.timed(PC_MISC, 0, [&] { return launch_conf_tokens(tokens, e->class_token, 1.f, 0.f, B, T, E, w.xc, s, true); }));
  } else {
    // LL -> BatchNorm2d(1) -> SELU -> class token
    GemmArgs ll = plain_gemm(w.ssl_h, kD, e->conf_ll, kD, B * T, E, kD);
    ll.bias = e->ll_b;
    ll.out_f = w.ll32; ll.ldo_f = E;
    KOK(cx.gemm(ll, dt, 1));
    KOK(cx.timed(PC_MISC, 0, [&] {
      return launch_conf_tokens(w.ll32, e->class_token, e->conf_bn_scale, e->conf_bn_shift, B, T, E, w.xc, s);
    }));
  }
  if (tap(cx, "tokens", w.xc, (size_t)M * E, false)) return 1;
  // K-padding columns of the operand buffers must read as zero (the fused chains only read past
  // the real columns of the attention output: 144 -> 160)
  const size_t hs = dtype_size(dt);
  // (split precision: the chains take fp32 operand rows and the pair-form weights; dt is DT_FP32 for every other kernel)
  const bool fused = e->fuse_conformer && (dt != DT_FP32 || e->s3) && E == 144 && e->inner == E && e->FFp == 4 * E && e->C2 == 2 * E;
  const int chain_dt = e->s3 ? DT_FP16X3 : dt;
  HIP_OK(hipMemsetAsync(w.ao, 0, (size_t)M * Ep * hs, s));
  if (!fused) {
    HIP_OK(hipMemsetAsync(w.hc, 0, (size_t)M * Ep * hs, s));
    HIP_OK(hipMemsetAsync(w.u, 0, (size_t)M * e->C2p * hs, s));
    if (e->FFp != e->FF) HIP_OK(hipMemsetAsync(w.hid, 0, (size_t)M * e->FFp * hs, s));
  }
  for (int b = 0; fused && b < e->nblk; ++b) {
    // three register-resident row chains around the attention and the depthwise conv
    const ConfBlock& K = e->blk[b];
    ConfChainArgs c;
    memset(&c, 0, sizeof c);
    c.M = M; c.E = E; c.Ep = Ep; c.FFp = e->FFp; c.objective = cx.objective;
    c.x_in = w.xc; c.x_out = w.xc;  // in place: a wave reads and writes only its own 16 rows
    auto ff = [&](const ConfFF& f) { c.ff_w1 = f.w1; c.ff_w2 = f.w2; };
    const double ff_fl = 2.0 * M * E * e->FF * 2;
    ff(K.ff[0]);
    c.params = K.chain_prm[0];
    c.w_a = K.wqkv; c.ld_w_a = Ep;
    c.out2 = w.qkv32; c.ld_out2 = 3 * e->inner;
    KOK(cx.timed(PC_CONF_CHAIN, ff_fl + 2.0 * M * E * 3 * e->inner, [&] { return launch_conf_chain(c, 0, chain_dt, s); }));
    auto bp = [b](const std::string& leaf) { return "b" + std::to_string(b) + "." + leaf; };  // (tap names: only while taps are on)
    TAP(bp("xa"), w.xc, (size_t)M * E, false, E);
    TAP(bp("qkv"), w.qkv32, (size_t)M * 3 * e->inner, false, 3 * e->inner);
    KOK(cx.timed(PC_CONF_ATTN, 6.0 * B * e->heads * (double)N * N * e->dh, [&] {
      if (e->conf_attn_mfma && dt != DT_FP32 && e->dh == 36)
        return launch_conf_attn_mfma(w.qkv32, 3 * e->inner, w.qkv32 + e->inner, 3 * e->inner, K.rel_h, 512, B, N, e->heads,
                                     e->dh, w.ao, Ep, dt, s, w.lens, 1);
      if (e->conf_attn_mfma && e->s3 && e->dh == 36 && N <= 209)  // split precision: the one-pass kernel on hi / lo halves, fp32 rows out
        return launch_conf_attn_split(w.qkv32, 3 * e->inner, w.qkv32 + e->inner, 3 * e->inner, (const float*)K.rel_h, 512, B, N,
                                      e->heads, e->dh, (float*)w.ao, Ep, s, w.lens, 1);
      return launch_conf_attn(w.qkv32, 3 * e->inner, w.qkv32 + e->inner, 3 * e->inner,
                              K.rel32, 512, B, N, e->heads, e->dh, w.ao, Ep, dt, s, w.lens, 1);
    }));
    TAP(bp("ao"), w.ao, (size_t)M * Ep, true, Ep);
    c.in_h = w.ao; c.ld_in_h = Ep;
    c.params = K.chain_prm[1];
    c.w_a = K.wout;
    c.w_b = K.pw1;
    c.out2 = w.glu32; c.ld_out2 = 2 * e->C2;
    KOK(cx.timed(PC_CONF_CHAIN, 2.0 * M * E * (e->inner + 2 * e->C2), [&] { return launch_conf_chain(c, 1, chain_dt, s); }));
    TAP(bp("xb"), w.xc, (size_t)M * E, false, E);
    TAP(bp("glu"), w.glu32, (size_t)M * 2 * e->C2, false, 2 * e->C2);
    KOK(cx.timed(PC_CONF_DWCONV, 2.0 * B * N * e->C2 * e->ck, [&] {
      return launch_conf_dwconv(w.glu32, 2 * e->C2, K.dw_w, K.dw_b, K.bn_scale, K.bn_shift, B, N, e->C2, e->ck, w.u, e->C2p, dt, s, w.lens, 1);
    }));
    TAP(bp("u"), w.u, (size_t)M * e->C2p, true, e->C2p);
    c.in_h = w.u; c.ld_in_h = e->C2p;
    c.params = K.chain_prm[2];
    c.w_a = K.pw2; c.ld_w_a = e->C2p;
    ff(K.ff[1]);
    c.w_b = nullptr; c.out2 = nullptr;
    KOK(cx.timed(PC_CONF_CHAIN, ff_fl + 2.0 * M * e->C2 * E, [&] { return launch_conf_chain(c, 2, chain_dt, s); }));
    if (e->taps_on) {
      const std::string nm = "block" + std::to_string(b);
      if (tap(cx, nm.c_str(), w.xc, (size_t)M * E, false)) return 1;
    }
  }
  for (int b = 0; !fused && b < e->nblk; ++b) {
    const ConfBlock& K = e->blk[b];
    auto bp = [b](const std::string& leaf) { return "b" + std::to_string(b) + "." + leaf; };  // (tap names: only while taps are on)
    auto norm_to_h = [&](const LnW& ln) -> const char* {
      RowNormArgs n = plain_norm(w.xc, E, M, E);
      n.out_h = w.hc; n.ldo_h = Ep;
      return cx.rownorm(n, ln, dt);
    };
    auto feed_forward = [&](const char* ff, const ConfFF& f) -> int {
      KOK(norm_to_h(f.ln));
      TAP(bp(std::string(ff) + ".hc"), w.hc, (size_t)M * Ep, true, Ep);
      GemmArgs a = plain_gemm(w.hc, Ep, f.w1, Ep, M, e->FF, Ep);
      a.k_algo = E;
      a.bias = f.b1; a.act = ACT_SWISH;
      a.out_h = w.hid; a.ldo_h = e->FFp;
      KOK(cx.gemm(a, dt, 1));
      TAP(bp(std::string(ff) + ".hid"), w.hid, (size_t)M * e->FFp, true, e->FFp);
      GemmArgs c = plain_gemm(w.hid, e->FFp, f.w2, e->FFp, M, E, e->FFp);
      c.k_algo = e->FF;
      c.bias = f.b2; c.alpha = 0.5f;
      c.resid = w.xc; c.ldr = E; c.out_f = w.xc; c.ldo_f = E;
      KOK(cx.gemm(c, dt, 1));
      return 0;
    };
    if (feed_forward("ff1", K.ff[0])) return 1;
    TAP(bp("xa"), w.xc, (size_t)M * E, false, E);
    // attention
    KOK(norm_to_h(K.attn_ln));
    TAP(bp("attn.hc"), w.hc, (size_t)M * Ep, true, Ep);
    GemmArgs q = plain_gemm(w.hc, Ep, K.wqkv, Ep, M, 3 * e->inner, Ep);
    q.k_algo = E;
    q.out_f = w.qkv32; q.ldo_f = 3 * e->inner;
    KOK(cx.gemm(q, dt, 1));
    TAP(bp("qkv"), w.qkv32, (size_t)M * 3 * e->inner, false, 3 * e->inner);
    KOK(cx.timed(PC_CONF_ATTN, 6.0 * B * e->heads * (double)N * N * e->dh, [&] {
      if (e->conf_attn_mfma && dt != DT_FP32 && e->dh == 36)
        return launch_conf_attn_mfma(w.qkv32, 3 * e->inner, w.qkv32 + e->inner, 3 * e->inner, K.rel_h, 512, B, N, e->heads,
                                     e->dh, w.ao, Ep, dt, s, w.lens, 1);
      if (e->conf_attn_mfma && e->s3 && e->dh == 36 && N <= 209)  // split precision: the one-pass kernel on hi / lo halves, fp32 rows out
        return launch_conf_attn_split(w.qkv32, 3 * e->inner, w.qkv32 + e->inner, 3 * e->inner, (const float*)K.rel_h, 512, B, N,
                                      e->heads, e->dh, (float*)w.ao, Ep, s, w.lens, 1);
      return launch_conf_attn(w.qkv32, 3 * e->inner, w.qkv32 + e->inner, 3 * e->inner,
                              K.rel32, 512, B, N, e->heads, e->dh, w.ao, Ep, dt, s, w.lens, 1);
    }));
    TAP(bp("ao"), w.ao, (size_t)M * Ep, true, Ep);
    GemmArgs o = plain_gemm(w.ao, Ep, K.wout, Ep, M, E, Ep);
    o.k_algo = e->inner;
    o.bias = K.bout;
    o.resid = w.xc; o.ldr = E; o.out_f = w.xc; o.ldo_f = E;
    KOK(cx.gemm(o, dt, 1));
    TAP(bp("xb"), w.xc, (size_t)M * E, false, E);
    // conv module
    KOK(norm_to_h(K.conv_ln));
    TAP(bp("conv.hc"), w.hc, (size_t)M * Ep, true, Ep);
    GemmArgs p1 = plain_gemm(w.hc, Ep, K.pw1, Ep, M, 2 * e->C2, Ep);
    p1.k_algo = E;
    p1.bias = K.bpw1;
    p1.out_f = w.glu32; p1.ldo_f = 2 * e->C2;
    KOK(cx.gemm(p1, dt, 1));
    TAP(bp("glu"), w.glu32, (size_t)M * 2 * e->C2, false, 2 * e->C2);
    KOK(cx.timed(PC_CONF_DWCONV, 2.0 * B * N * e->C2 * e->ck, [&] {
      return launch_conf_dwconv(w.glu32, 2 * e->C2, K.dw_w, K.dw_b, K.bn_scale, K.bn_shift, B, N, e->C2, e->ck, w.u, e->C2p, dt, s, w.lens, 1);
    }));
    TAP(bp("u"), w.u, (size_t)M * e->C2p, true, e->C2p);
    GemmArgs p2 = plain_gemm(w.u, e->C2p, K.pw2, e->C2p, M, E, e->C2p);
    p2.k_algo = e->C2;
    p2.bias = K.bpw2;
    p2.resid = w.xc; p2.ldr = E; p2.out_f = w.xc; p2.ldo_f = E;
    KOK(cx.gemm(p2, dt, 1));
    TAP(bp("xc"), w.xc, (size_t)M * E, false, E);
    if (feed_forward("ff2", K.ff[1])) return 1;
    TAP(bp("xd"), w.xc, (size_t)M * E, false, E);
    RowNormArgs pn = plain_norm(w.xc, E, M, E);
    pn.out_f = w.xc; pn.ldo_f = E;
    KOK(cx.rownorm(pn, K.post_ln, dt));
    if (e->taps_on) {
      const std::string nm = "block" + std::to_string(b);
      if (tap(cx, nm.c_str(), w.xc, (size_t)M * E, false)) return 1;
    }
  }
  KOK(cx.timed(PC_MISC, 0, [&] {
    return launch_small_linear(w.xc, (long)N * E, B, E, e->fc5_w, e->fc5_b, 2,
                               logits, s, e->nonfinite + 1);
  }));
  if (embedding)  // x[:, 0, :] (models/conformer_baseline.py:27)
    HIP_OK(hipMemcpy2DAsync(embedding, (size_t)E * 4, w.xc, (size_t)N * E * 4, (size_t)E * 4, B, hipMemcpyDeviceToDevice, s));
  return 0;
}

static int run_head(Call& cx, int B, int T, Ws& w, float* logits) {
  afx_engine* e = cx.e;
  const hipStream_t s = cx.s;
  if (e->cfg.arch == AFX_ARCH_CONFORMER) return run_conformer(cx, B, T, w, logits);
  if (e->cfg.arch == AFX_ARCH_XLSR_AASIST) {
    // taps on: the back-end hands every launch's output to tap() before a later launch overwrites it
    w.aa.tap = e->taps_on ? +[](void* c, const char* nm, const float* p, size_t n) { return tap(*(Call*)c, nm, p, n, false); } : nullptr;
    w.aa.tap_ctx = e->taps_on ? &cx : nullptr;
    const char* m = cx.timed(PC_AASIST, 2.0 * B * 1.399e9 / 2, [&] { return aasist_forward(e->aw, w.ssl_f, B, T, w.aa, logits, s, e->nonfinite + 1); });
    w.aa.tap = nullptr;
    w.aa.tap_ctx = nullptr;
    if (m) return fail("%s", m);
    if (e->taps_on) {
      if (tap(cx, "logits", logits, (size_t)B * 2, false)) return 1;
      if (tap(cx, "e_S", w.aa.eS, (size_t)B * 42 * 64, false)) return 1;
      if (tap(cx, "e_T", w.aa.eT, (size_t)B * (T / 3) * 64, false)) return 1;
      if (tap(cx, "hidden", w.aa.hidden, (size_t)B * 160, false)) return 1;
      for (int i = 0; i < w.aa.dbg_count; ++i)
        if (tap(cx, w.aa.dbg_name[i], w.aa.dbg_ptr[i], w.aa.dbg_n[i], false)) return 1;
    }
    return 0;
  }
  return fail("afx_forward: this handle is an SSL feature extractor; use afx_ssl_forward");
}

__global__ void f32_to_half_kernel(const float* in, uint16_t* out, size_t n, int is_bf16);  // (defined below)

// ---------------------------------------------------------------------------------
// KV-cached streaming mode (BASELINE config 5 as named: "250 ms chunks with cached SSL-encoder KV state").
// NOT A REFERENCE FUNCTION.  The reference's trunk is bidirectional over the clip (full self-attention, a centred
// k = 128 positional conv, models/fe.py:17-21), so an encoder that sees every frame ONCE, when its chunk arrives, is
// a different model; SURVEY.md section 7 scopes it as a labelled mode whose parity target is this build's own offline
// restatement of the same function (oracle/streaming.py), not the reference.  The function, per chunk c of n_c frames
// (the frames of conv layer 6 that became computable with the chunk's samples):
//   * conv feature extractor, feature LayerNorm, projection: frame-local -- exact;
//   * positional conv: frame t of chunk c sees projected frames [t - 64, end of chunk c] (left context cached, the
//     right context beyond the chunk is zero, as beyond a clip's end);
//   * every transformer layer: the chunk's frames are the queries; keys / values are the chunk itself and the cached
//     K / V of the 15 chunks before it (16 chunks = 4 s of context), written once when their chunk passed;
//   * final LayerNorm; the back-end (AASIST / Conformer head) scores the window of the last <= 200 feature frames.
// State per stream: 24 x 256 x 3072 halfs of [q | k | v] rows (16-slot groups, one per chunk), 64 projected frames, the
// feature window.  The whole step runs on new frames only: S x n_c rows through the products, one query tile per
// (stream, head) in the attention.
// The step has three entry points over ONE body (kv_trunk: feature LayerNorm .. final encoder LayerNorm).  An entry point
// checks its arguments, uploads its tables, describes itself to the body in a KvForm, then updates the windows and runs the
// back-end.  What a form supplies:
//                    afx_kv_step (lock-step)      afx_kv_step_ragged (sessions)    afx_kv_step_active (a list)
//   rows             S                            S                                A
//   history in       2-D copy                     2-D copy                         kv_hist_kernel by id
//   history out      2-D copy                     kv_hist_kernel (own n_s)         kv_hist_kernel by id
//   zero padding     past n                       past 64 + n_s (meta)             past 64 + n_i (meta)
//   QKV rows         ring row 16 group + r        ring row 16 group + r            row table: 256 ids[i] + 16 own group + r
//   ring attention   form 1: host cnt, group      form 2: tab, group               form 3: the list's table
//   final LayerNorm  into the other window        dense rows (w.fl)                dense rows (w.fl)
//                    buffer, after its shift
//   window update    (the shift above)            kv_feat_kernel, ping-pong        kv_shift_kernel, in place
//   back-end         uniform window, run_head     kv_score_windows                 kv_score_windows by id
// ---------------------------------------------------------------------------------
constexpr int kKvGroups = 16, kKvSlots = 256, kKvHist = 64, kKvFeat = 208, kKvWindow = 200;
struct afx_kv {
  afx_engine* e;
  int S;
  long hop = 0;
  int cnt[kKvGroups];
  int nfeat = 0, pp = 0;
  void* rings = nullptr;   // (layers, S, 256, 3072) operand type
  void* hist = nullptr;    // (S, 64, 1024) operand type: the newest projected frames (positional conv's left context)
  float* feat[2] = {nullptr, nullptr};  // (S, 208, 1024) fp32, right-aligned window, ping-pong
  // per-stream sessions (afx_kv_reset / afx_kv_step_ragged): once either is called, the state is per stream
  bool per_stream = false;
  // steps over a list of streams (afx_kv_step_active): from the first one on, the ring group is per stream ([1] of tab) and
  // each stream's window stays in feat[pp] (shifted in place); afx_kv_step_ragged then refuses the state
  bool active = false;
  int* tab = nullptr;    // device (S, 8) ints: [0] base group (the group of the stream's first chunk), [1] (active) its next group,
                         // bytes [16, 32) valid counts
  int* meta = nullptr;   // device (16 S) ints, written per call: frame counts | 64 + frame counts | window lengths | slot lists,
                         // (active steps) + back-end order | its stream ids | QKV row table | (8 A) the list's attention table
  std::vector<int> nfeat_s, hmeta;
};
struct KvWs {
  void *feats_h, *xpad, *hbuf, *att, *ff;
  float *xp, *x;
  float* fl = nullptr;  // per-stream step: the final LayerNorm's rows before they join each stream's window
  void* s3planes = nullptr;  // split precision: pair-form scratch of the chunk's products
  size_t s3bytes = 0;
  Ws head;
};
// what an entry point supplies to the shared body of the step (kv_trunk); the table above
struct KvForm {
  int rows;              // S, or the length of the list: M = rows x n
  const int* dn;         // device: frames per row block (null: every stream brings n) -- the history leaves by kv_hist_kernel
  const int* ids;        // device: the stream of each row block (a list; null: block b is stream b) -- the history also enters by it
  const int* pad_lens;   // device: 64 + frames per row block, the rows past them are zeroed (null: 64 + n)
  const int* qkv_rows;   // device: first ring row of each row block's chunk (a list); null: row 16 ring.q_tile of the block's own ring
  MhsaRingForm ring;
  float* win_next;       // lock-step: the window moves up by n into this buffer and the final LayerNorm writes the chunk's rows
                         // below it; null: the final LayerNorm writes dense rows into w.fl
};
static size_t kv_carve(const afx_engine* e, int S, int n, int Th, void* base, KvWs* k, bool per_stream = false) {
  Carver c(base);
  const size_t hs = dtype_size(e->dt), M = (size_t)S * n, Tp = kKvHist + n;
  k->feats_h = c.take(M * kC * hs);
  k->xpad = c.take((size_t)S * (Tp + kPosK) * kD * hs);
  k->xp = (float*)c.take((size_t)S * Tp * kD * 4);
  k->x = (float*)c.take(M * kD * 4);
  k->hbuf = c.take(M * kD * hs);
  k->att = c.take((size_t)S * 16 * kD * hs);
  k->ff = c.take(M * kF * hs);
  k->s3planes = nullptr;
  k->s3bytes = 0;
  if (e->s3) {
    k->s3bytes = c.largest + 4096;
    k->s3planes = c.take(k->s3bytes);
  }
  k->fl = per_stream ? (float*)c.take(M * kD * 4) : nullptr;
  c.off = (c.off + 255) & ~(size_t)255;
  const size_t head_bytes = carve(e, S, 0, Th, base ? (char*)base + c.off : nullptr, &k->head, 0, per_stream);
  return c.off + head_bytes + 256;
}
extern "C" int afx_kv_create(afx_handle h, int n_streams, afx_kv** out) {
  if (!h || !out || n_streams <= 0) return fail("afx_kv_create: bad argument");
  if (!h->finalized) return fail("afx_kv_create: weights not finalized");
  if (h->cfg.arch != AFX_ARCH_XLSR_AASIST && h->cfg.arch != AFX_ARCH_CONFORMER) return fail("afx_kv_create: a handle with a trunk and a back-end");
  if (h->dt == DT_FP32 && !h->s3) return fail("afx_kv_create: the KV-cached mode runs the half-precision kernels or split precision (fp16 / bf16 / fp16x3 engines)");
  if (h->cfg.extractor_mode != AFX_EXTRACTOR_LAYER_NORM || h->cfg.pre_emphasis) return fail("afx_kv_create: layer_norm extractor without fused pre-emphasis");
  afx_kv* k = new afx_kv();
  k->e = h;
  k->S = n_streams;
  for (int i = 0; i < kKvGroups; ++i) k->cnt[i] = 0;
  const size_t hs = h->hsz, ring = (size_t)h->cfg.n_layers * n_streams * kKvSlots * 3 * kD * hs, hist = (size_t)n_streams * kKvHist * kD * hs,
               feat = (size_t)n_streams * kKvFeat * kD * 4;
  bool ok = hipMalloc((void**)&k->tab, (size_t)n_streams * 32) == hipSuccess && hipMalloc((void**)&k->meta, (size_t)n_streams * 64) == hipSuccess &&
            hipMemset(k->tab, 0, (size_t)n_streams * 32) == hipSuccess &&
            hipMalloc(&k->rings, ring) == hipSuccess && hipMalloc(&k->hist, hist) == hipSuccess &&
            hipMalloc((void**)&k->feat[0], feat) == hipSuccess && hipMalloc((void**)&k->feat[1], feat) == hipSuccess;
  // the history starts as silence-before-the-stream (zero left padding); ring slots are masked until written
  ok = ok && hipMemset(k->rings, 0, ring) == hipSuccess && hipMemset(k->hist, 0, hist) == hipSuccess &&
       hipMemset(k->feat[0], 0, feat) == hipSuccess && hipMemset(k->feat[1], 0, feat) == hipSuccess;
  if (!ok) {
    (void)hipFree(k->rings); (void)hipFree(k->hist); (void)hipFree(k->feat[0]); (void)hipFree(k->feat[1]);
    (void)hipFree(k->tab); (void)hipFree(k->meta);
    delete k;
    return fail("afx_kv_create: device allocation failed (%zu bytes per stream)", (ring + hist + 2 * feat) / n_streams);
  }
  *out = k;
  return 0;
}
extern "C" void afx_kv_destroy(afx_kv* k) {
  if (!k) return;
  (void)hipFree(k->rings); (void)hipFree(k->hist); (void)hipFree(k->feat[0]); (void)hipFree(k->feat[1]);
  (void)hipFree(k->tab); (void)hipFree(k->meta);
  delete k;
}
extern "C" size_t afx_kv_state_bytes(const afx_kv* k) {
  if (!k) return 0;
  return (size_t)k->e->cfg.n_layers * k->S * kKvSlots * 3 * kD * k->e->hsz + (size_t)k->S * kKvHist * kD * k->e->hsz + 2 * (size_t)k->S * kKvFeat * kD * 4;
}
extern "C" size_t afx_kv_workspace_bytes(const afx_kv* k, int n_frames) {
  if (!k || n_frames <= 0 || n_frames > 16) return 0;
  KvWs w;
  return kv_carve(k->e, k->S, n_frames, kKvWindow, nullptr, &w);
}
// ---------------------------------------------------------------------------------
// Per-stream sessions (afx_kv_reset, afx_kv_step_ragged): streams that start at different ticks.  The ring group stays
// global (group = step % 16); per stream are its base group (where its first chunk sits), its valid counts, its frames per
// step (n_s <= n_max, rows padded to n_max) and its window length.  The ring attention visits the slots rotated by the base
// group, the key order of a stream that started at group 0: a session scores bit for bit as that stream alone from the start.
// ---------------------------------------------------------------------------------
__global__ void kv_reset_kernel(const int* __restrict__ slots, int* __restrict__ tab, int base_group, u32x4* __restrict__ hist,
                                long hist_words, u32x4* __restrict__ f0, u32x4* __restrict__ f1, long feat_words) {
  const long sl = slots[blockIdx.y];
  if (blockIdx.x == 0 && threadIdx.x == 0) {  // base_group < 0 (active steps): the new stream starts at the slot's own next group
    const int g = base_group >= 0 ? base_group : tab[sl * 8 + 1];
    for (int j = 0; j < 8; ++j) tab[sl * 8 + j] = j == 0 ? g : j == 1 && base_group < 0 ? g : 0;
  }
  const u32x4 z = {0u, 0u, 0u, 0u};
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < hist_words; i += (long)gridDim.x * blockDim.x) hist[sl * hist_words + i] = z;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < feat_words; i += (long)gridDim.x * blockDim.x) {
    f0[sl * feat_words + i] = z;
    f1[sl * feat_words + i] = z;
  }
}
__global__ void kv_count_kernel(int* __restrict__ tab, const int* __restrict__ n, int S, int group) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < S) ((unsigned char*)(tab + (long)b * 8 + 4))[group] = (unsigned char)n[b];
}
// hist[s] = rows [pad + n_s, pad + n_s + 64) of stream s's padded rows (the newest 64 projected frames); 16-byte words.
// ids (active steps): padded-row block b is stream ids[b]'s; gather != 0 copies the other way, hist[ids[b]] -> rows [pad, pad + 64)
__global__ void kv_hist_kernel(u32x4* __restrict__ hist, u32x4* __restrict__ xpad, const int* __restrict__ n, long row_words,
                               long xpad_rows, int pad, const int* __restrict__ ids, int gather) {
  const long b = blockIdx.y, sb = ids ? ids[b] : b;
  const long words = kKvHist * row_words;
  u32x4* rows = xpad + (b * xpad_rows + pad + (gather ? 0 : n[b])) * row_words;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += (long)gridDim.x * blockDim.x) {
    if (gather) rows[i] = hist[sb * words + i];
    else hist[sb * words + i] = rows[i];
  }
}
// the window moves up by n_s rows and the stream's n_s new feature rows (dense (S, n_max, 1024) fp32) join it right-aligned
__global__ void kv_feat_kernel(const f32x4* __restrict__ cur, f32x4* __restrict__ nxt, const f32x4* __restrict__ fl, const int* __restrict__ n, int n_max) {
  const long b = blockIdx.y;
  const int nb = n[b];
  constexpr long RW = kD / 4;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < kKvFeat * RW; i += (long)gridDim.x * blockDim.x) {
    const int r = (int)(i / RW), c = (int)(i % RW);
    nxt[b * kKvFeat * RW + i] = r < kKvFeat - nb ? cur[(b * kKvFeat + r + nb) * RW + c] : fl[(b * n_max + r - (kKvFeat - nb)) * RW + c];
  }
}
// out row i (pitch Tout rows) = the last th_i rows of the window of stream ids[i] (identity if null), LEFT-aligned, zeros after
__global__ void kv_gather_kernel(const f32x4* __restrict__ win, const int* __restrict__ ids, const int* __restrict__ th, int th_const,
                                 int Tout, f32x4* __restrict__ out) {
  const long i = blockIdx.y;
  const long b = ids ? ids[i] : i;
  const int t = th ? th[i] : th_const;
  constexpr long RW = kD / 4;
  for (long j = (long)blockIdx.x * blockDim.x + threadIdx.x; j < Tout * RW; j += (long)gridDim.x * blockDim.x) {
    const int r = (int)(j / RW), c = (int)(j % RW);
    out[i * Tout * RW + j] = r < t ? win[(b * kKvFeat + kKvFeat - t + r) * RW + c] : f32x4{0.f, 0.f, 0.f, 0.f};
  }
}
__global__ void kv_scatter_logits_kernel(const float* __restrict__ in, const int* __restrict__ ids, int nb, float* __restrict__ logits) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nb * 2) logits[(long)ids[i >> 1] * 2 + (i & 1)] = in[i];
}

// the lock-stepped state becomes per-stream tables (base group 0, the shared valid counts, the shared window length)
static int kv_to_per_stream(afx_kv* k, hipStream_t s) {
  if (k->per_stream) return 0;
  std::vector<int> t((size_t)k->S * 8, 0);
  for (int b = 0; b < k->S; ++b)
    for (int g = 0; g < kKvGroups; ++g) ((unsigned char*)&t[(size_t)b * 8 + 4])[g] = (unsigned char)k->cnt[g];
  HIP_OK(hipMemcpyAsync(k->tab, t.data(), t.size() * 4, hipMemcpyHostToDevice, s));
  HIP_OK(hipStreamSynchronize(s));  // (pageable host memory)
  k->nfeat_s.assign(k->S, k->nfeat);
  k->hmeta.assign((size_t)k->S * 4, 0);
  k->per_stream = true;
  return 0;
}

extern "C" int afx_kv_reset(afx_kv* k, const int* slots, int n_slots, void* stream) {
  if (!k || (n_slots > 0 && !slots) || n_slots < 0) return fail("afx_kv_reset: bad argument");
  std::vector<char> seen(k->S, 0);
  for (int i = 0; i < n_slots; ++i) {
    if (slots[i] < 0 || slots[i] >= k->S) return fail("afx_kv_reset: slot %d outside 0..%d", slots[i], k->S - 1);
    if (seen[slots[i]]++) return fail("afx_kv_reset: slot %d named twice", slots[i]);
  }
  hipStream_t s = (hipStream_t)stream;
  if (kv_to_per_stream(k, s)) return 1;
  if (n_slots == 0) return 0;
  for (int i = 0; i < n_slots; ++i) {
    k->nfeat_s[slots[i]] = 0;
    k->hmeta[(size_t)3 * k->S + i] = slots[i];
  }
  int* dslots = k->meta + 3 * k->S;
  HIP_OK(hipMemcpyAsync(dslots, k->hmeta.data() + 3 * k->S, (size_t)n_slots * 4, hipMemcpyHostToDevice, s));
  HIP_OK(hipStreamSynchronize(s));
  const size_t hs = k->e->hsz;
  hipLaunchKernelGGL(kv_reset_kernel, dim3(64, n_slots), dim3(256), 0, s, dslots, k->tab, k->active ? -1 : (int)(k->hop % kKvGroups), (u32x4*)k->hist,
                     (long)(kKvHist * kD * hs / 16), (u32x4*)k->feat[0], (u32x4*)k->feat[1], (long)(kKvFeat * kD * 4 / 16));
  HIP_OK(hipGetLastError());
  return 0;
}

// The two contexts of a step, each with the scratch and the buffer list of its own workspace.  chunk: the chunk's products take
// pair-form operands written by their producers, or converted into the chunk workspace's scratch (its buffers + the chunk's
// view of the padded rows); head: the back-end's products on the window.
struct KvCalls {
  Call chunk, head;
  KvCalls(afx_engine* e, void* stream, const KvWs& w)
      : chunk(e, stream, w.s3planes, w.s3bytes, {w.feats_h, w.hbuf, w.att, w.ff, w.xpad, (char*)w.xpad + (size_t)kKvHist * kD * e->hsz}),
        head(e, stream, w.head) {}
};
// The shared body of the three steps: the chunk's rows (f.rows blocks of n) from the feature LayerNorm to the final encoder
// LayerNorm.  Every difference between the forms is a field of KvForm.
// cx: the chunk's context (KvCalls::chunk)
static int kv_trunk(Call& cx, afx_kv* k, const KvForm& f, const float* feats6, int n, KvWs& w) {
  afx_engine* e = cx.e;
  const hipStream_t s = cx.s;
  const int R = f.rows, dt = e->dt, M = R * n, Tp = kKvHist + n;
  const size_t hs = e->hsz, xrow = (size_t)kD * hs, xpad_pitch = (size_t)(Tp + kPosK) * xrow;
  // feature LayerNorm -> operand type
  {
    RowNormArgs a = plain_norm(feats6, kC, M, kC);
    a.out_h = w.feats_h; a.ldo_h = kC;
    KOK(cx.rownorm(a, e->feat_ln, dt));
  }
  TAP("kv.feats", w.feats_h, (size_t)M * kC, true, kC);
  // positional conv operand: [64 zero rows | 64 cached projected frames | the chunk | 64 zero rows] per row block
  if (f.ids) {
    hipLaunchKernelGGL(kv_hist_kernel, dim3(32, R), dim3(256), 0, s, (u32x4*)k->hist, (u32x4*)w.xpad, f.dn, (long)(xrow / 16),
                       (long)(Tp + kPosK), kPosPad, f.ids, 1);
    HIP_OK(hipGetLastError());
  } else {
    HIP_OK(hipMemcpy2DAsync((char*)w.xpad + kPosPad * xrow, xpad_pitch, k->hist, kKvHist * xrow, kKvHist * xrow, R, hipMemcpyDeviceToDevice, s));
  }
  {
    GemmArgs g = plain_gemm(w.feats_h, kC, e->projw, kC, M, kD, kC);
    g.rpb = n; g.a_batch = (long)n * kC; g.a_row = kC;
    g.bias = e->proj_b;
    g.out_f = w.x; g.ldo_f = kD; g.o_batch_rows = n;  // the chunk's residual rows, dense (rows, n, 1024)
    g.out_h = w.xpad; g.ldo_h = kD; g.oh_batch_rows = Tp + kPosK; g.oh_row_off = kPosPad + kKvHist;
    KOK(cx.gemm(g, dt, 1));
    // (per-stream counts: a block's chunk rows past its own n_s are zero, as beyond its chunk when the stream steps alone)
    KOK(cx.timed(PC_MISC, 0, [&] { return launch_zero_pad_rows(w.xpad, R, Tp, kD, kPosPad, kPosK - kPosPad, dt, s, f.pad_lens); }));
  }
  TAP("kv.xpad", w.xpad, (size_t)R * (Tp + kPosK) * kD, true, kD);  // (the whole padded buffer of every row block, pad rows included)
  TAP("kv.proj", w.x, (size_t)M * kD, false, kD);
  // The positional conv of the chunk's n frames ONLY (round 4: it used to run over all 64 + n rows of the padded layout and
  // keep the last n -- 6x the work at n = 13): output frame j reads rows [64 + j, 192 + j) of the block's padded rows, i.e. rows
  // [j, j + 128) from the first cached frame on.
  void* xchunk = (char*)w.xpad + (size_t)kKvHist * xrow;
  if (!e->s3) {
    PosConvArgs pc;
    memset(&pc, 0, sizeof pc);
    pc.xpad = xchunk; pc.xpad_batch = (long)(Tp + kPosK) * kD; pc.W = e->posw; pc.bias = e->pos_b;
    pc.x = w.x; pc.B = R; pc.T = n;
    KOK(cx.timed(PC_POSCONV, 2.0 * R * n * kD * (kD / kPosG) * kPosK, [&] { return launch_posconv(pc, dt, s); }));
  } else {  // split precision: the grouped product of run_trunk
    cx.s3_set(xchunk, kS3ScaleFree);  // (history rows copied in above + the rows the projection just wrote: pair form, scale 1)
    KOK(posconv_product(cx, xchunk, Tp + kPosK, R, n, w.x, dt));
  }
  TAP("kv.pos", w.x, (size_t)M * kD, false, kD);
  // the newest 64 projected frames become the next chunk's left context
  if (f.dn) {
    hipLaunchKernelGGL(kv_hist_kernel, dim3(32, R), dim3(256), 0, s, (u32x4*)k->hist, (u32x4*)w.xpad, f.dn, (long)(xrow / 16),
                       (long)(Tp + kPosK), kPosPad, f.ids, 0);
    HIP_OK(hipGetLastError());
  } else {
    HIP_OK(hipMemcpy2DAsync(k->hist, kKvHist * xrow, (char*)w.xpad + (size_t)(kPosPad + n) * xrow, xpad_pitch, kKvHist * xrow, R, hipMemcpyDeviceToDevice, s));
  }
  for (int l = 0; l < e->cfg.n_layers; ++l) {
    const TrunkLayer& L = e->layers[l];
    void* ring = (char*)k->rings + (size_t)l * k->S * kKvSlots * 3 * kD * hs;
    auto lp = [l](const char* leaf) { return "kv.l" + std::to_string(l) + "." + leaf; };  // (tap names: built only while taps are on)
    RowNormArgs n1 = plain_norm(w.x, kD, M, kD);
    n1.out_h = w.hbuf; n1.ldo_h = kD;
    KOK(cx.rownorm(n1, L.ln1, dt));
    TAP(lp("ln1"), w.hbuf, (size_t)M * kD, true, kD);
    // q | k | v of the chunk go straight into its 16-slot group of the ring (row remap or row table of the epilogue): K / V are
    // cached by being written
    GemmArgs q = plain_gemm(w.hbuf, kD, L.wqkv, kD, M, 3 * kD, kD);
    q.rpb = n; q.a_batch = (long)n * kD; q.a_row = kD;
    q.bias = L.bqkv;
    q.out_h = ring; q.ldo_h = 3 * kD;
    if (f.qkv_rows) {
      q.oh_rows = f.qkv_rows;
    } else {
      q.oh_batch_rows = kKvSlots; q.oh_row_off = f.ring.q_tile * 16;
    }
    KOK(cx.gemm(q, dt, 1, f.qkv_rows != nullptr));
    TAP(lp("ring"), ring, (size_t)k->S * kKvSlots * 3 * kD, true, 3 * kD);  // (this layer's whole ring, every stream of the state)
    KOK(cx.timed(PC_MHSA, 4.0 * R * kH * 16.0 * kKvSlots * 64, [&] {
      if (e->s3) {  // fp32 [q | k | v] slots, hi / lo pairs split in the kernel; the output leaves as the output projection's pair-form operand
        const bool pairs = cx.s3_ok(w.att);
        cx.s3_set(w.att, pairs ? kS3ScaleFree : 0.f);
        return launch_mhsa_ring_split((const float*)ring, (float*)w.att, R, kH, f.ring, s, pairs, kS3ScaleFree);
      }
      return launch_mhsa_ring(ring, w.att, R, kH, f.ring, dt, s);
    }));
    TAP(lp("att"), w.att, (size_t)R * 16 * kD, true, kD);  // (a 16-row block per row block)
    GemmArgs o = plain_gemm(w.att, kD, L.wo, kD, M, kD, kD);
    o.rpb = n; o.a_batch = 16L * kD; o.a_row = kD; o.o_batch_rows = n;
    o.bias = L.bo; o.resid = w.x; o.ldr = kD; o.out_f = w.x; o.ldo_f = kD;
    KOK(cx.gemm(o, dt, 1));
    TAP(lp("mid"), w.x, (size_t)M * kD, false, kD);
    RowNormArgs n2 = plain_norm(w.x, kD, M, kD);
    n2.out_h = w.hbuf; n2.ldo_h = kD;
    KOK(cx.rownorm(n2, L.ln2, dt));
    TAP(lp("ln2"), w.hbuf, (size_t)M * kD, true, kD);
    GemmArgs f1 = plain_gemm(w.hbuf, kD, L.w1, kD, M, kF, kD);
    f1.bias = L.b1; f1.act = ACT_GELU; f1.out_h = w.ff; f1.ldo_h = kF;
    KOK(cx.gemm(f1, dt, 1));
    TAP(lp("ff"), w.ff, (size_t)M * kF, true, kF);
    GemmArgs f2 = plain_gemm(w.ff, kF, L.w2, kF, M, kD, kF);
    f2.bias = L.b2; f2.resid = w.x; f2.ldr = kD; f2.out_f = w.x; f2.ldo_f = kD;
    KOK(cx.gemm(f2, dt, 1));
    TAP("kv.layer" + std::to_string(l), w.x, (size_t)M * kD, false, kD);
  }
  RowNormArgs nf = plain_norm(w.x, kD, M, kD);
  if (f.win_next) {
    const size_t frow = (size_t)kD * 4, fpitch = (size_t)kKvFeat * frow;
    HIP_OK(hipMemcpy2DAsync(f.win_next, fpitch, (char*)k->feat[k->pp] + (size_t)n * frow, fpitch, (size_t)(kKvFeat - n) * frow, R, hipMemcpyDeviceToDevice, s));
    nf.out_f = f.win_next; nf.ldo_f = kD; nf.rpb = n; nf.o_batch_rows = kKvFeat; nf.o_row_off = kKvFeat - n;
  } else {
    nf.out_f = w.fl; nf.ldo_f = kD;
  }
  nf.nonfinite = e->nonfinite;
  KOK(cx.rownorm(nf, e->enc_ln, dt));
  if (!f.win_next) TAP("kv.fl", w.fl, (size_t)M * kD, false, kD);  // (lock-step: the rows are the last n of every stream's "kv.win")
  return 0;
}

// feats6: device (S, n, 512) fp32 -- the n NEW frames of conv layer 6 (conv + LayerNorm + GELU applied: what the conv stack
// hands the feature LayerNorm), 1 <= n <= 16.  logits: device (S, 2): the back-end's logits on the window that ends with this chunk.
extern "C" int afx_kv_step(afx_kv* k, const float* feats6, int n, float* logits, void* ws, size_t ws_bytes, void* stream) {
  if (n < 1 || n > 16) return fail("afx_kv_step: a chunk brings 1..16 frames (got %d)", n);
  if (!k || !feats6 || !logits || !ws) return fail("afx_kv_step: null argument");
  if (k->active) return fail("afx_kv_step: this state holds per-stream ring positions (afx_kv_step_active): continue with afx_kv_step_active");
  if (k->per_stream) return fail("afx_kv_step: this state holds per-stream sessions (afx_kv_reset / afx_kv_step_ragged): continue with afx_kv_step_ragged");
  afx_engine* e = k->e;
  const int S = k->S, dt = e->dt, group = (int)(k->hop % kKvGroups);
  const int Th = std::min(k->nfeat + n, kKvWindow);
  if (e->cfg.arch == AFX_ARCH_XLSR_AASIST && Th < 6) return fail("afx_kv_step: the AASIST head needs at least 6 frames in the window");
  KvWs w;
  const size_t needb = kv_carve(e, S, n, Th, ws, &w);
  if (ws_bytes < needb) return fail("afx_kv_step: workspace too small (%zu < %zu bytes)", ws_bytes, needb);
  KvCalls calls(e, stream, w);
  Call& cx = calls.chunk;
  const hipStream_t s = cx.s;
  k->cnt[group] = n;
  // the chunk's features join the right-aligned window (old frames move up by n in the other buffer)
  float* nxt = k->feat[k->pp ^ 1];
  KvForm f = {};
  f.rows = S;
  f.ring = MhsaRingForm{1, group, k->cnt, nullptr};
  f.win_next = nxt;
  if (kv_trunk(cx, k, f, feats6, n, w)) return 1;
  TAP("kv.win", nxt, (size_t)S * kKvFeat * kD, false, kD);
  k->pp ^= 1;
  k->nfeat = std::min(k->nfeat + n, kKvFeat);
  // back-end on the window of the last Th frames
  const size_t frow = (size_t)kD * 4, fpitch = (size_t)kKvFeat * frow;
  HIP_OK(hipMemcpy2DAsync(w.head.ssl_f, (size_t)Th * frow, (char*)nxt + (size_t)(kKvFeat - Th) * frow, fpitch, (size_t)Th * frow, S, hipMemcpyDeviceToDevice, s));
  if (e->cfg.arch == AFX_ARCH_CONFORMER) {
    if (e->s3) {  // (fp32 operand buffers: the head's LL converts the rows it reads into its own scratch)
      HIP_OK(hipMemcpyAsync(w.head.ssl_h, w.head.ssl_f, (size_t)S * Th * kD * 4, hipMemcpyDeviceToDevice, s));
    } else {
      hipLaunchKernelGGL(f32_to_half_kernel, dim3(1024), dim3(256), 0, s, w.head.ssl_f, (uint16_t*)w.head.ssl_h, (size_t)S * Th * kD, dt == AFX_DT_BF16 ? 1 : 0);
      HIP_OK(hipGetLastError());
    }
  }
  k->hop += 1;
  if (e->taps_on && tap(cx, "ssl", w.head.ssl_f, (size_t)S * Th * kD, false)) return 1;
  return run_head(calls.head, S, Th, w.head, logits);
}

// AASIST scores uniform batches: the entries grouped by window length (one sub-batch each, as afx_forward_ragged does).
// order = the entries sorted by length (stable); returns (length, first position in the order) per bucket
static std::vector<std::pair<int, int>> kv_buckets(const int* th, int count, int* order) {
  std::vector<std::pair<int, int>> buckets;
  for (int i = 0; i < count; ++i) order[i] = i;
  std::stable_sort(order, order + count, [&](int a, int c) { return th[a] < th[c]; });
  for (int i = 0; i < count; ++i)
    if (i == 0 || th[order[i]] != th[order[i - 1]]) buckets.push_back({th[order[i]], i});
  return buckets;
}

// The back-end of the per-stream steps: entry i of `count` scores the last dth[i] (<= Thmax) rows of its stream's window in `win`
struct KvWindows {
  const float* win;
  int count, Thmax;
  const int *ids, *dth;      // device.  Conformer, every window left-aligned in one batch with key-padding lengths
                             // (afx_forward_ragged's head): entry i is stream ids[i] (null: stream i), its length dth[i]
  const int *b_ids, *b_row;  // device.  AASIST, the bucket loop: position j of the order is stream b_ids[j], logits row b_row[j]
  std::vector<std::pair<int, int>> buckets;  // AASIST: kv_buckets
};
// cx: the back-end's context (KvCalls::head)
static int kv_score_windows(Call& cx, KvWs& w, const KvWindows& v, float* logits) {
  afx_engine* e = cx.e;
  const hipStream_t s = cx.s;
  const int count = v.count, Thmax = v.Thmax;
  if (e->cfg.arch == AFX_ARCH_CONFORMER) {
    hipLaunchKernelGGL(kv_gather_kernel, dim3(32, count), dim3(256), 0, s, (const f32x4*)v.win, v.ids, v.dth, 0, Thmax, (f32x4*)w.head.ssl_f);
    HIP_OK(hipGetLastError());
    TAP("ssl", w.head.ssl_f, (size_t)count * Thmax * kD, false, kD);  // (the head's input: every window left-aligned, zeros after)
    HIP_OK(hipMemcpyAsync(w.head.lens, v.dth, (size_t)count * 4, hipMemcpyDeviceToDevice, s));
    if (e->s3) {  // (fp32 operand buffers: the head's LL converts the rows it reads into its own scratch)
      HIP_OK(hipMemcpyAsync(w.head.ssl_h, w.head.ssl_f, (size_t)count * Thmax * kD * 4, hipMemcpyDeviceToDevice, s));
    } else {
      hipLaunchKernelGGL(f32_to_half_kernel, dim3(1024), dim3(256), 0, s, w.head.ssl_f, (uint16_t*)w.head.ssl_h, (size_t)count * Thmax * kD, e->dt == AFX_DT_BF16 ? 1 : 0);
      HIP_OK(hipGetLastError());
    }
    return run_head(cx, count, Thmax, w.head, logits);
  }
  for (size_t bi = 0; bi < v.buckets.size(); ++bi) {
    const int t = v.buckets[bi].first, i0 = v.buckets[bi].second;
    const int nb = (bi + 1 < v.buckets.size() ? v.buckets[bi + 1].second : count) - i0;
    hipLaunchKernelGGL(kv_gather_kernel, dim3(32, nb), dim3(256), 0, s, (const f32x4*)v.win, v.b_ids + i0, (const int*)nullptr, t, t, (f32x4*)w.head.bucket_f);
    HIP_OK(hipGetLastError());
    TAP("kv.bucket" + std::to_string(bi), w.head.bucket_f, (size_t)nb * t * kD, false, kD);
    if (const char* m = aasist_forward(e->aw, w.head.bucket_f, nb, t, w.head.aa, w.head.bucket_logits, s, e->nonfinite + 1)) return fail("%s", m);
    hipLaunchKernelGGL(kv_scatter_logits_kernel, dim3((2 * nb + 255) / 256), dim3(256), 0, s, w.head.bucket_logits, v.b_row + i0, nb, logits);
    HIP_OK(hipGetLastError());
  }
  return 0;
}

extern "C" size_t afx_kv_ragged_workspace_bytes(const afx_kv* k, int n_max) {
  if (!k || n_max <= 0 || n_max > 16) return 0;
  KvWs w;
  return kv_carve(k->e, k->S, n_max, kKvWindow, nullptr, &w, true);
}

// feats6: device (S, n_max, 512) fp32, stream b's n_frames[b] new frames first (rows past them are read but never score);
// n_frames: host, S entries, 1 <= n_frames[b] <= n_max <= 16.  Same function per stream as afx_kv_step on that stream alone.
extern "C" int afx_kv_step_ragged(afx_kv* k, const float* feats6, int n, const int* n_frames, float* logits, void* ws, size_t ws_bytes,
                                  void* stream) {
  if (n < 1 || n > 16) return fail("afx_kv_step_ragged: a chunk brings 1..16 frames (got n_max %d)", n);
  if (!k || !feats6 || !n_frames || !logits || !ws) return fail("afx_kv_step_ragged: null argument");
  if (k->active) return fail("afx_kv_step_ragged: this state holds per-stream ring positions (afx_kv_step_active): continue with afx_kv_step_active");
  afx_engine* e = k->e;
  const int S = k->S, group = (int)(k->hop % kKvGroups);
  for (int b = 0; b < S; ++b)
    if (n_frames[b] < 1 || n_frames[b] > n) return fail("afx_kv_step_ragged: stream %d brings %d frames (1..%d)", b, n_frames[b], n);
  hipStream_t s = (hipStream_t)stream;
  if (kv_to_per_stream(k, s)) return 1;
  int Thmax = 0;
  std::vector<int>& hm = k->hmeta;  // meta: n | 64 + n | window lengths | back-end order
  for (int b = 0; b < S; ++b) {
    const int th = std::min(k->nfeat_s[b] + n_frames[b], kKvWindow);
    if (e->cfg.arch == AFX_ARCH_XLSR_AASIST && th < 6) return fail("afx_kv_step_ragged: the AASIST head needs at least 6 frames in stream %d's window", b);
    hm[b] = n_frames[b];
    hm[S + b] = kKvHist + n_frames[b];
    hm[2 * S + b] = th;
    Thmax = std::max(Thmax, th);
  }
  KvWs w;
  const size_t needb = kv_carve(e, S, n, Thmax, ws, &w, true);
  if (ws_bytes < needb) return fail("afx_kv_step_ragged: workspace too small (%zu < %zu bytes)", ws_bytes, needb);
  KvCalls calls(e, stream, w);
  Call& cx = calls.chunk;
  const int* dn = k->meta;
  KvWindows v = {nullptr, S, Thmax, nullptr, dn + 2 * S, dn + 3 * S, dn + 3 * S, {}};  // (every stream, in place; scores in bucket order)
  if (e->cfg.arch == AFX_ARCH_XLSR_AASIST) v.buckets = kv_buckets(&hm[2 * S], S, &hm[3 * S]);
  HIP_OK(hipMemcpyAsync(k->meta, hm.data(), (size_t)S * 16, hipMemcpyHostToDevice, s));
  HIP_OK(hipStreamSynchronize(s));  // (pageable host memory)
  hipLaunchKernelGGL(kv_count_kernel, dim3((S + 255) / 256), dim3(256), 0, s, k->tab, dn, S, group);
  HIP_OK(hipGetLastError());
  KvForm f = {};
  f.rows = S;
  f.dn = dn;
  f.pad_lens = dn + S;
  f.ring = MhsaRingForm{2, group, nullptr, k->tab};
  if (kv_trunk(cx, k, f, feats6, n, w)) return 1;
  float *cur = k->feat[k->pp], *nxt = k->feat[k->pp ^ 1];
  hipLaunchKernelGGL(kv_feat_kernel, dim3(64, S), dim3(256), 0, s, (const f32x4*)cur, (f32x4*)nxt, (const f32x4*)w.fl, dn, n);
  HIP_OK(hipGetLastError());
  TAP("kv.win", nxt, (size_t)S * kKvFeat * kD, false, kD);
  k->pp ^= 1;
  for (int b = 0; b < S; ++b) k->nfeat_s[b] = std::min(k->nfeat_s[b] + n_frames[b], kKvFeat);
  k->hop += 1;
  v.win = nxt;
  return kv_score_windows(calls.head, w, v, logits);
}

// ---------------------------------------------------------------------------------
// Steps over a list of active streams (afx_kv_step_active): only the listed streams advance, the others keep every byte of
// their state.  The ring group is per stream from the first such step on -- tab[8 s + 1] is stream s's next group, its base
// group plus its own step count mod 16 -- so a stream's chunks still fill consecutive groups from its base and the rotated
// visit gives the key order of a fresh stream.  Everything runs on the A x n dense rows of the list; state is reached by id.
// ---------------------------------------------------------------------------------
// every stream's next group = the lock-stepped group (the first active step of a state)
__global__ void kv_activate_kernel(int* __restrict__ tab, int S, int group) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < S) tab[(long)b * 8 + 1] = group;
}
// list entry i (stream ids[i], n[i] new frames): its group's valid count, its attention-table row ([0] base, [1] group, [2] id,
// [4, 8) counts), its QKV row offset; then the stream's next group moves on
__global__ void kv_active_tab_kernel(int* __restrict__ tab, const int* __restrict__ ids, const int* __restrict__ n, int A,
                                     int* __restrict__ atab, int* __restrict__ rows) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A) return;
  const long sl = ids[i];
  int* t = tab + sl * 8;
  const int g = t[1];
  ((unsigned char*)(t + 4))[g] = (unsigned char)n[i];
  for (int j = 0; j < 8; ++j) atab[(long)i * 8 + j] = j == 1 ? g : j == 2 ? (int)sl : t[j];
  rows[i] = (int)(sl * kKvSlots + g * 16);
  t[1] = (g + 1) % kKvGroups;
}
// stream ids[i]'s window moves up by n[i] rows IN PLACE and entry i's new rows (dense (A, n_max, 1024) fp32) join it at the
// bottom.  Columns are independent: block x owns 32 16-byte columns of the stream and walks its rows downward-to-upward in
// passes of 8 -- a pass reads rows [r0 + n, r0 + n + 8) into registers, waits for the whole block, then writes rows [r0, r0 + 8);
// a later pass only reads rows below every row written so far, so no read meets a rewritten row.
__global__ void kv_shift_kernel(f32x4* __restrict__ win, const f32x4* __restrict__ fl, const int* __restrict__ ids, const int* __restrict__ n,
                                int n_max) {
  constexpr int RW = kD / 4;
  static_assert(kKvFeat % 8 == 0 && RW % 32 == 0, "pass shape");
  const long i = blockIdx.y;
  const int nb = n[i], c = blockIdx.x * 32 + (threadIdx.x & 31), rr = threadIdx.x >> 5;  // 256 threads = 8 rows x 32 columns
  f32x4* w = win + (long)ids[i] * kKvFeat * RW;
  for (int r0 = 0; r0 < kKvFeat; r0 += 8) {
    const int r = r0 + rr;
    const f32x4 v = r + nb < kKvFeat ? w[(long)(r + nb) * RW + c] : fl[(i * n_max + r + nb - kKvFeat) * RW + c];
    __syncthreads();
    w[(long)r * RW + c] = v;
  }
}

extern "C" size_t afx_kv_active_workspace_bytes(const afx_kv* k, int n_active, int n_max) {
  if (!k || n_active <= 0 || n_active > k->S || n_max <= 0 || n_max > 16) return 0;
  KvWs w;
  return kv_carve(k->e, n_active, n_max, kKvWindow, nullptr, &w, true);
}

// slots: host, A distinct stream indices (the list, in the caller's order); feats6: device (A, n_max, 512) fp32, entry i's
// n_frames[i] (host, 1 <= n_frames[i] <= n_max <= 16) new frames first; logits: device (A, 2) in list order.
extern "C" int afx_kv_step_active(afx_kv* k, const int* slots, int A, const float* feats6, int n, const int* n_frames, float* logits,
                                  void* ws, size_t ws_bytes, void* stream) {
  if (!k) return fail("afx_kv_step_active: null state");
  if (A < 0 || A > k->S) return fail("afx_kv_step_active: %d active streams (0..%d)", A, k->S);
  if (A == 0) return 0;  // nothing advances, nothing is launched
  if (n < 1 || n > 16) return fail("afx_kv_step_active: a chunk brings 1..16 frames (got n_max %d)", n);
  if (!slots || !feats6 || !n_frames || !logits || !ws) return fail("afx_kv_step_active: null argument");
  afx_engine* e = k->e;
  const int S = k->S;
  {
    std::vector<char> seen(S, 0);
    for (int i = 0; i < A; ++i) {
      if (slots[i] < 0 || slots[i] >= S) return fail("afx_kv_step_active: slot %d outside 0..%d", slots[i], S - 1);
      if (seen[slots[i]]++) return fail("afx_kv_step_active: slot %d named twice", slots[i]);
      if (n_frames[i] < 1 || n_frames[i] > n) return fail("afx_kv_step_active: slot %d brings %d frames (1..%d)", slots[i], n_frames[i], n);
    }
  }
  int Thmax = 0;
  std::vector<int> th(A);
  for (int i = 0; i < A; ++i) {
    th[i] = std::min((k->per_stream ? k->nfeat_s[slots[i]] : k->nfeat) + n_frames[i], kKvWindow);
    if (e->cfg.arch == AFX_ARCH_XLSR_AASIST && th[i] < 6) return fail("afx_kv_step_active: the AASIST head needs at least 6 frames in slot %d's window", slots[i]);
    Thmax = std::max(Thmax, th[i]);
  }
  KvWs w;
  const size_t needb = kv_carve(e, A, n, Thmax, ws, &w, true);
  if (ws_bytes < needb) return fail("afx_kv_step_active: workspace too small (%zu < %zu bytes)", ws_bytes, needb);
  KvCalls calls(e, stream, w);
  Call& cx = calls.chunk;
  const hipStream_t s = cx.s;
  if (kv_to_per_stream(k, s)) return 1;
  if (!k->active) {  // every stream's next group = the group a lock-stepped or ragged step would write now
    hipLaunchKernelGGL(kv_activate_kernel, dim3((S + 255) / 256), dim3(256), 0, s, k->tab, S, (int)(k->hop % kKvGroups));
    HIP_OK(hipGetLastError());
    k->active = true;
  }
  // meta: n | 64 + n | window lengths | ids | back-end order (list entries) | their ids | QKV rows | (8 A) attention table
  std::vector<int> hm((size_t)6 * A, 0);
  for (int i = 0; i < A; ++i) {
    hm[i] = n_frames[i];
    hm[A + i] = kKvHist + n_frames[i];
    hm[2 * A + i] = th[i];
    hm[3 * A + i] = slots[i];
  }
  int* dn = k->meta;
  const int *dids = dn + 3 * A, *drows = dn + 6 * A, *datab = dn + 8 * A;
  KvWindows v = {k->feat[k->pp], A, Thmax, dids, dn + 2 * A, dn + 5 * A, dn + 4 * A, {}};  // (active steps: every window stays in this buffer)
  if (e->cfg.arch == AFX_ARCH_XLSR_AASIST) {
    v.buckets = kv_buckets(th.data(), A, &hm[4 * A]);
    for (int i = 0; i < A; ++i) hm[5 * A + i] = slots[hm[4 * A + i]];
  }
  HIP_OK(hipMemcpyAsync(dn, hm.data(), (size_t)6 * A * 4, hipMemcpyHostToDevice, s));
  HIP_OK(hipStreamSynchronize(s));  // (pageable host memory)
  hipLaunchKernelGGL(kv_active_tab_kernel, dim3((A + 255) / 256), dim3(256), 0, s, k->tab, dids, dn, A, dn + 8 * A, dn + 6 * A);
  HIP_OK(hipGetLastError());
  KvForm f = {};
  f.rows = A;
  f.dn = dn;
  f.ids = dids;
  f.pad_lens = dn + A;
  f.qkv_rows = drows;
  f.ring = MhsaRingForm{3, 0, nullptr, datab};
  if (kv_trunk(cx, k, f, feats6, n, w)) return 1;
  hipLaunchKernelGGL(kv_shift_kernel, dim3(kD / 4 / 32, A), dim3(256), 0, s, (f32x4*)k->feat[k->pp], (const f32x4*)w.fl, dids, dn, n);
  HIP_OK(hipGetLastError());
  TAP("kv.win", k->feat[k->pp], (size_t)S * kKvFeat * kD, false, kD);  // (every stream of the state: the unnamed ones keep every byte)
  for (int i = 0; i < A; ++i) k->nfeat_s[slots[i]] = std::min(k->nfeat_s[slots[i]] + n_frames[i], kKvFeat);
  return kv_score_windows(calls.head, w, v, logits);
}

// ---------------------------------------------------------------------------------
// Moving sessions (afx_kv_export / afx_kv_import): a stream's state leaves one afx_kv as a payload and enters a slot of
// another (or of the same one, on another GPU, after host memory).  Payload per stream, 16-byte words:
//   [n_layers x 256 ring rows x the k | v thirds (2 x 1024 operand-type elements)] [64 x 1024 operand type: the positional
//   conv's context] [208 x 1024 fp32: the feature window of feat[pp]]
// Ring rows go in the stream's own order: payload group j is ring group (base + j) & 15.  The host meta row (AFX_KV_META
// ints) holds the layout word, the next group relative to the base, the window length and the 16 valid counts in the same
// relative order.  Import picks the destination's base so that the stream's next chunk lands where the destination writes
// next (its global group; an active-list state takes the same group as the stream's next one): the per-stream attention
// forms visit the keys rotated by the base, so the summation order, and every bit, is the one the stream had.
// Only k and v move.  The q third of a ring row is read by the ring attention for the query tile alone (RING == 1:
// ring.q_tile, RING == 2: the step's group, RING == 3: the stream's own group, tab[1]) -- the group the same step's QKV
// product has just written -- and for keys only the k / v thirds are loaded (afx_attn.hip, mhsa_kernel and
// mhsa_split_kernel).  A q row of an older group is never read again, so the destination's q columns stay as they are.
// ---------------------------------------------------------------------------------
constexpr int kKvFormat = 1;
static size_t kv_slot_bytes(const afx_engine* e) {
  return (size_t)e->cfg.n_layers * kKvSlots * 2 * kD * e->hsz + (size_t)kKvHist * kD * e->hsz + (size_t)kKvFeat * kD * 4;
}
// n_layers | dtype << 8 | element size << 12 | 256 / 16 - 1 << 16 | 64 / 16 << 20 | 208 / 16 << 24 | format << 28
static int kv_layout_word(const afx_engine* e) {
  static_assert(kKvSlots % 16 == 0 && kKvSlots / 16 <= 16 && kKvHist % 16 == 0 && kKvHist / 16 < 16 && kKvFeat % 16 == 0 &&
                kKvFeat / 16 < 16 && kKvFormat < 8, "layout word fields");
  return (e->cfg.n_layers & 0xff) | (e->dt & 0xf) << 8 | ((int)e->hsz & 0xf) << 12 | (kKvSlots / 16 - 1) << 16 | (kKvHist / 16) << 20 |
         (kKvFeat / 16) << 24 | kKvFormat << 28;
}
// One launch per call over the slot list: block row i moves stream ids[i] (ring group of payload group j = (base_i + j) & 15,
// base_i = bases[i], or tab[8 ids[i]] when bases is null, or 0 when both are null: a lock-stepped state).  rs = log2 of the
// k | v words of a ring row (256 or 512).  IMPORT: payload -> state, and tab row ids[i] = rows[8 i .. 8 i + 8).
template <bool IMPORT>
__global__ __launch_bounds__(256) void kv_move_kernel(u32x4* __restrict__ rings, u32x4* __restrict__ hist, u32x4* __restrict__ win,
                                                      u32x4* __restrict__ payload, const int* __restrict__ ids, const int* __restrict__ bases,
                                                      int* __restrict__ tab, const int* __restrict__ rows, int S, int n_layers, int rs,
                                                      long hist_words, long win_words) {
  const long i = blockIdx.y, sl = ids[i];
  const int base = bases ? bases[i] : tab ? tab[sl * 8] : 0;
  const long row_words = 1L << rs, ring_words = (long)n_layers * kKvSlots << rs;
  u32x4* p = payload + i * (ring_words + hist_words + win_words);
  const long stride = (long)gridDim.x * blockDim.x, t0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  // four independent words per thread and pass: the loads are issued before the stores
  for (long w0 = t0; w0 < ring_words; w0 += 4 * stride) {
    u32x4 v[4];
    long at[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long w = w0 + u * stride;
      const long r = w >> rs, l = r / kKvSlots;
      const int rr = (int)(r % kKvSlots), g = ((rr >> 4) + base) & (kKvGroups - 1);
      // [q | k | v] ring row = 3 / 2 row_words words; k | v start at its second third
      at[u] = w < ring_words ? ((l * S + sl) * kKvSlots + g * 16 + (rr & 15)) * (3 * row_words / 2) + row_words / 2 + (w & (row_words - 1)) : -1;
      if (at[u] >= 0) v[u] = IMPORT ? p[w] : rings[at[u]];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (at[u] < 0) continue;
      if (IMPORT) rings[at[u]] = v[u];
      else p[w0 + u * stride] = v[u];
    }
  }
  u32x4 *ph = p + ring_words, *pw = ph + hist_words, *h = hist + sl * hist_words, *f = win + sl * win_words;
  for (long w = t0; w < hist_words; w += stride) {
    if (IMPORT) h[w] = ph[w];
    else ph[w] = h[w];
  }
  for (long w = t0; w < win_words; w += stride) {
    if (IMPORT) f[w] = pw[w];
    else pw[w] = f[w];
  }
  if (IMPORT && blockIdx.x == 0 && threadIdx.x < 8) tab[sl * 8 + threadIdx.x] = rows[i * 8 + threadIdx.x];
}

static int kv_slot_list(const afx_kv* k, const int* slots, int n, const char* what) {
  std::vector<char> seen(k->S, 0);
  for (int i = 0; i < n; ++i) {
    if (slots[i] < 0 || slots[i] >= k->S) return fail("%s: slot %d outside 0..%d", what, slots[i], k->S - 1);
    if (seen[slots[i]]++) return fail("%s: slot %d named twice", what, slots[i]);
  }
  return 0;
}
static int kv_move_launch(afx_kv* k, bool import, int n, void* payload, const int* bases, hipStream_t s) {
  const afx_engine* e = k->e;
  if (n > 65535) return fail("afx_kv_%s: at most 65535 streams per call", import ? "import" : "export");
  const int rs = e->hsz == 4 ? 9 : 8;  // 2 x 1024 elements of 2 or 4 bytes = 256 or 512 words
  const int gx = std::max(8, std::min(256, 4096 / n));
  u32x4* win = (u32x4*)k->feat[k->pp];
  const long hw = (long)kKvHist * kD * e->hsz / 16, ww = (long)kKvFeat * kD * 4 / 16;
  if (import)
    hipLaunchKernelGGL(kv_move_kernel<true>, dim3(gx, n), dim3(256), 0, s, (u32x4*)k->rings, (u32x4*)k->hist, win, (u32x4*)payload, k->meta,
                       bases, k->tab, k->meta + 2 * n, k->S, e->cfg.n_layers, rs, hw, ww);
  else
    hipLaunchKernelGGL(kv_move_kernel<false>, dim3(gx, n), dim3(256), 0, s, (u32x4*)k->rings, (u32x4*)k->hist, win, (u32x4*)payload, k->meta,
                       (const int*)nullptr, k->per_stream ? k->tab : nullptr, (const int*)nullptr, k->S, e->cfg.n_layers, rs, hw, ww);
  HIP_OK(hipGetLastError());
  return 0;
}

extern "C" size_t afx_kv_slot_bytes(const afx_kv* k) { return k ? kv_slot_bytes(k->e) : 0; }

extern "C" int afx_kv_export(afx_kv* k, const int* slots, int n, void* payload, int* meta, void* stream) {
  if (!k) return fail("afx_kv_export: null state");
  if (n < 0 || n > k->S) return fail("afx_kv_export: %d streams (0..%d)", n, k->S);
  if (n == 0) return 0;
  if (!slots || !payload || !meta) return fail("afx_kv_export: null argument");
  if ((uintptr_t)payload & 15) return fail("afx_kv_export: the payload must be 16-byte aligned");
  if (kv_slot_list(k, slots, n, "afx_kv_export")) return 1;
  hipStream_t s = (hipStream_t)stream;
  // the state is read, never converted: a lock-stepped state exports base 0, its shared counts, group and window length
  std::vector<int> t;
  if (k->per_stream) {
    t.resize((size_t)k->S * 8);
    HIP_OK(hipMemcpyAsync(t.data(), k->tab, t.size() * 4, hipMemcpyDeviceToHost, s));
  }
  std::vector<int> ids(slots, slots + n);
  HIP_OK(hipMemcpyAsync(k->meta, ids.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
  HIP_OK(hipStreamSynchronize(s));
  const int layout = kv_layout_word(k->e), group = (int)(k->hop % kKvGroups);
  for (int i = 0; i < n; ++i) {
    const int* row = k->per_stream ? &t[(size_t)slots[i] * 8] : nullptr;
    const int base = row ? row[0] & (kKvGroups - 1) : 0, next = row && k->active ? row[1] : group;
    int* m = meta + (size_t)i * AFX_KV_META;
    m[0] = layout;
    m[1] = (next - base) & (kKvGroups - 1);
    m[2] = k->per_stream ? k->nfeat_s[slots[i]] : k->nfeat;
    m[3] = 0;
    unsigned char* c = (unsigned char*)(m + 4);
    for (int j = 0; j < kKvGroups; ++j)
      c[j] = row ? ((const unsigned char*)(row + 4))[(base + j) & (kKvGroups - 1)] : (unsigned char)k->cnt[(base + j) & (kKvGroups - 1)];
  }
  return kv_move_launch(k, false, n, payload, nullptr, s);
}

extern "C" int afx_kv_import(afx_kv* k, const int* slots, int n, const void* payload, const int* meta, void* stream) {
  if (!k) return fail("afx_kv_import: null state");
  if (n < 0 || n > k->S) return fail("afx_kv_import: %d streams (0..%d)", n, k->S);
  if (n == 0) return 0;
  if (!slots || !payload || !meta) return fail("afx_kv_import: null argument");
  if ((uintptr_t)payload & 15) return fail("afx_kv_import: the payload must be 16-byte aligned");
  if (kv_slot_list(k, slots, n, "afx_kv_import")) return 1;
  const int layout = kv_layout_word(k->e);
  for (int i = 0; i < n; ++i) {  // every row is checked before anything changes
    const int* m = meta + (size_t)i * AFX_KV_META;
    if (m[0] != layout)
      return fail("afx_kv_import: stream %d's layout word 0x%08x does not match this state's 0x%08x (layers, dtype, element size, "
                  "ring / context / window rows, format)", i, (unsigned)m[0], (unsigned)layout);
    if (m[1] < 0 || m[1] >= kKvGroups || m[2] < 0 || m[2] > kKvFeat || m[3] != 0) return fail("afx_kv_import: stream %d's meta row is corrupt", i);
    for (int j = 0; j < kKvGroups; ++j)
      if (((const unsigned char*)(m + 4))[j] > 16) return fail("afx_kv_import: stream %d holds a group of more than 16 frames", i);
  }
  hipStream_t s = (hipStream_t)stream;
  if (kv_to_per_stream(k, s)) return 1;  // (a never-reset lock-stepped state becomes per stream, as afx_kv_reset makes it)
  // the stream's next chunk goes where this state writes next: the global group (an active-list state: the same group,
  // set as the stream's own next one)
  const int group = (int)(k->hop % kKvGroups);
  std::vector<int> h((size_t)10 * n, 0);
  for (int i = 0; i < n; ++i) {
    const int* m = meta + (size_t)i * AFX_KV_META;
    const int base = (group - m[1]) & (kKvGroups - 1);
    h[i] = slots[i];
    h[n + i] = base;
    int* row = &h[(size_t)2 * n + 8 * i];
    row[0] = base;
    row[1] = group;
    for (int j = 0; j < kKvGroups; ++j) ((unsigned char*)(row + 4))[(base + j) & (kKvGroups - 1)] = ((const unsigned char*)(m + 4))[j];
  }
  HIP_OK(hipMemcpyAsync(k->meta, h.data(), h.size() * 4, hipMemcpyHostToDevice, s));
  HIP_OK(hipStreamSynchronize(s));  // (pageable host memory)
  if (kv_move_launch(k, true, n, const_cast<void*>(payload), k->meta + n, s)) return 1;
  for (int i = 0; i < n; ++i) k->nfeat_s[slots[i]] = meta[(size_t)i * AFX_KV_META + 2];
  return 0;
}

static int check_call(afx_handle h, const void* in, int B, int L, const void* out, void* ws, bool needs_trunk = false) {
  if (!h || !in || !out || !ws) return fail("afx: null argument");
  if (needs_trunk && h->cfg.arch == AFX_ARCH_CONFORMER_HEAD) return fail("afx: this handle holds Conformer blocks only (MyConformer); use afx_conformer_forward");
  if (!h->finalized) return fail("afx: weights not finalized (call afx_finalize after afx_load_weight)");
  if (B <= 0 || L <= 0) return fail("afx: empty batch (B=%d, L=%d)", B, L);
  return 0;
}
// ... then carves the caller's workspace (carve's own arguments) and refuses one that is too small
static int carve_ws(const char* who, afx_handle h, int B, int L, int Th, void* ws, size_t ws_bytes, Ws* w, int T5 = 0, bool ragged = false) {
  const size_t needb = carve(h, B, L, Th, ws, w, T5, ragged);
  return ws_bytes < needb ? fail("%s: workspace too small (%zu < %zu bytes)", who, ws_bytes, needb) : 0;
}

extern "C" int afx_forward(afx_handle h, const float* wave, int B, int L, float* logits, void* ws, size_t ws_bytes,
                           void* stream) {
  if (check_call(h, wave, B, L, logits, ws, true)) return 1;
  Ws w;
  if (carve_ws("afx_forward", h, B, L, 0, ws, ws_bytes, &w)) return 1;
  Call cx(h, stream, w);
  if (run_trunk(cx, wave, B, L, w)) return 1;
  return run_head(cx, B, w.T[6], w, logits);
}

// The forward in two halves, so that a scoring loop can run the back-end of batch i on a second stream under the trunk of
// batch i+1 (the AASIST head is 11 % of the teacher's time on at most 132 workgroups: alone it leaves half the chip idle):
// afx_trunk_forward leaves the SSL features in the workspace, afx_head_from_workspace runs the back-end on them.  The caller
// orders the two calls (an event between the streams) and alternates two workspaces; same kernels, same bits as afx_forward.
extern "C" int afx_trunk_forward(afx_handle h, const float* wave, int B, int L, void* ws, size_t ws_bytes, void* stream) {
  if (check_call(h, wave, B, L, ws, ws, true)) return 1;
  Ws w;
  if (carve_ws("afx_trunk_forward", h, B, L, 0, ws, ws_bytes, &w)) return 1;
  Call cx(h, stream, w);
  return run_trunk(cx, wave, B, L, w);
}
extern "C" int afx_head_from_workspace(afx_handle h, int B, int L, float* logits, void* ws, size_t ws_bytes, void* stream) {
  if (check_call(h, ws, B, L, logits, ws, true)) return 1;
  if (h->cfg.arch == AFX_ARCH_SSL) return fail("afx_head_from_workspace: this handle has no back-end");
  Ws w;
  if (carve_ws("afx_head_from_workspace", h, B, L, 0, ws, ws_bytes, &w)) return 1;
  if (w.T[6] < 1) return fail("afx_head_from_workspace: %d samples are too few for one output frame", L);
  Call cx(h, stream, w);
  // split precision: the Conformer head's LL reads the features' operand copy, which the trunk's final LayerNorm wrote as
  // pair-form rows (run_trunk: Call::rownorm).  That was afx_trunk_forward's call; this one starts from what the workspace holds
  if (cx.s3_ok(w.ssl_h)) cx.s3_set(w.ssl_h, h->enc_ln.scale);
  return run_head(cx, B, w.T[6], w, logits);
}

// The path from the output of conv layer 5 on (conv layer 6, feature LayerNorm, projection, positional conv,
// transformer layers, head): what a streaming caller runs every hop after it has produced only the NEW frames of
// conv layers 0-5 (afx/streaming.py).  Same kernels, same order as afx_forward from that point on.
extern "C" size_t afx_tail_workspace_bytes(afx_handle h, int B, int T5) {
  if (!h || B <= 0 || T5 <= 0) return 0;
  Ws w;
  return carve(h, B, 0, 0, nullptr, &w, T5);
}
extern "C" int afx_tail_forward_strided(afx_handle h, const void* conv5_h, long batch_stride, int B, int T5, float* logits,
                                        void* ws, size_t ws_bytes, void* stream) {
  if (check_call(h, conv5_h, B, T5, logits, ws)) return 1;
  if (h->cfg.arch == AFX_ARCH_SSL || h->cfg.arch == AFX_ARCH_CONFORMER_HEAD) return fail("afx_tail_forward: this handle has no trunk + back-end");
  if (batch_stride != 0 && batch_stride < (long)T5 * kC) return fail("afx_tail_forward_strided: batch stride %ld is shorter than a window (%ld)", batch_stride, (long)T5 * kC);
  if (batch_stride % 8) return fail("afx_tail_forward_strided: the batch stride must keep rows 16-byte aligned");
  if (h->s3 && batch_stride != 0 && batch_stride != (long)T5 * kC) return fail("afx_tail_forward_strided: split precision reads a packed window");
  Ws w;
  if (carve_ws("afx_tail_forward", h, B, 0, 0, ws, ws_bytes, &w, T5)) return 1;
  if (w.T[6] < 1) return fail("afx_tail_forward: %d conv-layer-5 frames are too few for one output frame", T5);
  Call cx(h, stream, w);
  if (run_trunk(cx, nullptr, B, 0, w, conv5_h, batch_stride)) return 1;
  return run_head(cx, B, w.T[6], w, logits);
}
extern "C" int afx_tail_forward(afx_handle h, const void* conv5_h, int B, int T5, float* logits, void* ws, size_t ws_bytes,
                                void* stream) {
  return afx_tail_forward_strided(h, conv5_h, 0, B, T5, logits, ws, ws_bytes, stream);
}

// The tail over windows at arbitrary frame offsets of one shared layer-5 buffer (afx/timeline.py: the conv stack runs
// once over a whole recording, the windows of many recordings overlap in one buffer).  A gather kernel packs the B
// windows into the workspace -- a plain 16-byte copy -- and the packed tail above runs on them unchanged.  The offsets
// travel as kernel arguments, kGatherMax per launch: nothing is uploaded and the call stays asynchronous.
constexpr int kGatherMax = 64;
struct GatherArgs {
  const uint4* src;
  uint4* dst;
  long long n16;                // 16-byte vectors per window
  long long off16[kGatherMax];  // window starts in the source, in 16-byte vectors
};
__global__ __launch_bounds__(256) void gather_windows_kernel(GatherArgs a) {
  const int b = blockIdx.y;
  const uint4* __restrict__ src = a.src + a.off16[b];
  uint4* __restrict__ dst = a.dst + (long long)b * a.n16;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < a.n16; i += (long long)gridDim.x * blockDim.x)
    dst[i] = src[i];
}
static size_t packed_windows_bytes(const afx_engine* e, int B, int T5) {
  return ((size_t)B * T5 * kC * dtype_size(e->dt) + 255) & ~(size_t)255;
}
extern "C" size_t afx_tail_windows_workspace_bytes(afx_handle h, int B, int T5) {
  if (!h || B <= 0 || T5 <= 0) return 0;
  Ws w;
  return packed_windows_bytes(h, B, T5) + carve(h, B, 0, 0, nullptr, &w, T5);
}
extern "C" int afx_tail_forward_windows(afx_handle h, const void* conv5_h, long long total_elems, const long long* offs, int B,
                                        int T5, float* logits, void* ws, size_t ws_bytes, void* stream) {
  if (check_call(h, conv5_h, B, T5, logits, ws)) return 1;
  if (!offs) return fail("afx_tail_forward_windows: null offsets");
  if (h->cfg.arch == AFX_ARCH_SSL || h->cfg.arch == AFX_ARCH_CONFORMER_HEAD) return fail("afx_tail_forward_windows: this handle has no trunk + back-end");
  if ((uintptr_t)conv5_h & 15) return fail("afx_tail_forward_windows: the layer-5 buffer must be 16-byte aligned");
  if ((uintptr_t)ws & 15) return fail("afx_tail_forward_windows: the workspace must be 16-byte aligned");
  const long long win = (long long)T5 * kC;
  for (int b = 0; b < B; ++b) {
    if (offs[b] < 0 || offs[b] % 8)
      return fail("afx_tail_forward_windows: offset %lld of window %d is not a non-negative multiple of 8 elements", offs[b], b);
    if (offs[b] > total_elems - win)
      return fail("afx_tail_forward_windows: window %d (%lld + %lld elements) reaches past the buffer's %lld", b, offs[b], win,
                  total_elems);
  }
  const size_t hs = dtype_size(h->dt), packed = packed_windows_bytes(h, B, T5);
  Ws w;
  const size_t needb = packed + carve(h, B, 0, 0, (char*)ws + packed, &w, T5);
  if (ws_bytes < needb) return fail("afx_tail_forward_windows: workspace too small (%zu < %zu bytes)", ws_bytes, needb);
  if (w.T[6] < 1) return fail("afx_tail_forward_windows: %d conv-layer-5 frames are too few for one output frame", T5);
  hipStream_t s = (hipStream_t)stream;
  GatherArgs g;
  g.src = (const uint4*)conv5_h;
  g.n16 = win * (long long)hs / 16;
  const long long per_row = (g.n16 + 255) / 256;
  for (int b0 = 0; b0 < B; b0 += kGatherMax) {
    const int nb = B - b0 < kGatherMax ? B - b0 : kGatherMax;
    for (int i = 0; i < nb; ++i) g.off16[i] = offs[b0 + i] * (long long)hs / 16;
    g.dst = (uint4*)ws + (long long)b0 * g.n16;
    // about 2048 workgroups per launch whatever the batch: a few per CU, each lane a handful of 16-byte copies
    const long long gx = std::max(1LL, std::min(per_row, 2048LL / nb));
    hipLaunchKernelGGL(gather_windows_kernel, dim3((unsigned)gx, nb), dim3(256), 0, s, g);
    HIP_OK(hipGetLastError());
  }
  Call cx(h, stream, w);
  if (run_trunk(cx, nullptr, B, 0, w, ws, 0)) return 1;
  return run_head(cx, B, w.T[6], w, logits);
}

// ---------------------------------------------------------------------------------
// ragged batches: clips of different lengths in ONE forward, each scored exactly as if alone.
// The conv stack is local and unpadded, so frame t of a clip depends on its first 400 + 320 t samples only: a clip
// zero-padded to the batch's longest gives its own T_b frames unchanged, followed by frames nobody may look at.
// "Nobody looks" = key-padding masks (attention keys beyond T_b staged as zeros and masked to -1e30: they contribute
// exactly 0), zeros in the positional conv's operand copy and in the depthwise conv's input beyond T_b, and the
// class token / logits taken per utterance.  Everything else on the path is row-local.  The AASIST graph back-end has
// per-utterance graph sizes (T_b / 3 temporal nodes): it runs once per distinct length on the gathered sub-batch.
// ---------------------------------------------------------------------------------
static int ragged_setup(afx_engine* h, int B, int Lmax, const int* n_samples, Ws& w, std::vector<int>& frames, hipStream_t s) {
  frames.resize(B);
  for (int b = 0; b < B; ++b) {
    if (n_samples[b] > Lmax) return fail("afx_forward_ragged: clip %d has %d samples, the batch rows hold %d", b, n_samples[b], Lmax);
    int T[7];
    conv_lengths(n_samples[b], T);
    if (T[6] < 1) return fail("afx_forward_ragged: clip %d has %d samples, too few for one output frame (need >= 400)", b, n_samples[b]);
    frames[b] = T[6];
  }
  HIP_OK(hipMemcpyAsync(w.lens, frames.data(), (size_t)B * 4, hipMemcpyHostToDevice, s));
  HIP_OK(hipStreamSynchronize(s));  // `frames` is pageable host memory: the copy must have read it before it dies
  return 0;
}

extern "C" size_t afx_ragged_workspace_bytes(afx_handle h, int B, int Lmax) {
  if (!h || B <= 0 || Lmax <= 0) return 0;
  Ws w;
  return carve(h, B, Lmax, 0, nullptr, &w, 0, true);
}

extern "C" int afx_forward_ragged(afx_handle h, const float* wave, int B, int Lmax, const int* n_samples, float* logits,
                                  void* ws, size_t ws_bytes, void* stream) {
  if (check_call(h, wave, B, Lmax, logits, ws, true)) return 1;
  if (!n_samples) return fail("afx_forward_ragged: null lengths");
  if (h->cfg.arch == AFX_ARCH_SSL) return fail("afx_forward_ragged: this handle is an SSL feature extractor; use afx_ssl_forward_ragged");
  if (h->cfg.pre_emphasis) return fail("afx_forward_ragged: engine-side pre-emphasis is not supported on ragged batches");
  if (h->cfg.extractor_mode == AFX_EXTRACTOR_GROUP_NORM) return fail("afx_forward_ragged: the group-norm extractor normalises over the whole clip; zero padding would enter its statistics");
  Ws w;
  if (carve_ws("afx_forward_ragged", h, B, Lmax, 0, ws, ws_bytes, &w, 0, true)) return 1;
  hipStream_t s = (hipStream_t)stream;
  std::vector<int> frames;
  if (ragged_setup(h, B, Lmax, n_samples, w, frames, s)) return 1;
  Call cx(h, stream, w);
  if (run_trunk(cx, wave, B, Lmax, w)) return 1;
  const int Tmax = w.T[6];
  if (h->cfg.arch == AFX_ARCH_CONFORMER) return run_head(cx, B, Tmax, w, logits);
  // AASIST: one uniform sub-batch per distinct length
  std::vector<char> done(B, 0);
  for (int b0 = 0; b0 < B; ++b0) {
    if (done[b0]) continue;
    const int t = frames[b0];
    std::vector<int> idx;
    for (int b = b0; b < B; ++b)
      if (!done[b] && frames[b] == t) { idx.push_back(b); done[b] = 1; }
    const int nb = (int)idx.size();
    for (int k = 0; k < nb; ++k)
      HIP_OK(hipMemcpyAsync(w.bucket_f + (size_t)k * t * kD, w.ssl_f + (size_t)idx[k] * Tmax * kD, (size_t)t * kD * 4,
                            hipMemcpyDeviceToDevice, s));
    if (const char* m = aasist_forward(h->aw, w.bucket_f, nb, t, w.aa, w.bucket_logits, s, h->nonfinite + 1)) return fail("%s", m);
    for (int k = 0; k < nb; ++k)
      HIP_OK(hipMemcpyAsync(logits + (size_t)idx[k] * 2, w.bucket_logits + (size_t)k * 2, 8, hipMemcpyDeviceToDevice, s));
  }
  return 0;
}

// feats: device (B,Tmax,1024) fp32, rows past an utterance's own frame count are zeroed; n_frames (host int[B], may be
// null) receives the frame counts
extern "C" int afx_ssl_forward_ragged(afx_handle h, const float* wave, int B, int Lmax, const int* n_samples, float* feats,
                                      int* n_frames, void* ws, size_t ws_bytes, void* stream) {
  if (check_call(h, wave, B, Lmax, feats, ws, true)) return 1;
  if (!n_samples) return fail("afx_ssl_forward_ragged: null lengths");
  if (h->cfg.pre_emphasis) return fail("afx_ssl_forward_ragged: engine-side pre-emphasis is not supported on ragged batches");
  if (h->cfg.extractor_mode == AFX_EXTRACTOR_GROUP_NORM) return fail("afx_ssl_forward_ragged: the group-norm extractor normalises over the whole clip; zero padding would enter its statistics");
  Ws w;
  if (carve_ws("afx_ssl_forward_ragged", h, B, Lmax, 0, ws, ws_bytes, &w, 0, true)) return 1;
  hipStream_t s = (hipStream_t)stream;
  std::vector<int> frames;
  if (ragged_setup(h, B, Lmax, n_samples, w, frames, s)) return 1;
  Call cx(h, stream, w);
  if (run_trunk(cx, wave, B, Lmax, w)) return 1;
  const int Tmax = w.T[6];
  HIP_OK(hipMemcpyAsync(feats, w.ssl_f, (size_t)B * Tmax * kD * 4, hipMemcpyDeviceToDevice, s));
  for (int b = 0; b < B; ++b) {
    if (frames[b] < Tmax)
      HIP_OK(hipMemsetAsync(feats + ((size_t)b * Tmax + frames[b]) * kD, 0, (size_t)(Tmax - frames[b]) * kD * 4, s));
    if (n_frames) n_frames[b] = frames[b];
  }
  return 0;
}

extern "C" int afx_ssl_forward(afx_handle h, const float* wave, int B, int L, float* feats, void* ws, size_t ws_bytes,
                               void* stream) {
  if (check_call(h, wave, B, L, feats, ws, true)) return 1;
  Ws w;
  if (carve_ws("afx_ssl_forward", h, B, L, 0, ws, ws_bytes, &w)) return 1;
  hipStream_t s = (hipStream_t)stream;
  Call cx(h, stream, w);
  if (run_trunk(cx, wave, B, L, w)) return 1;
  HIP_OK(hipMemcpyAsync(feats, w.ssl_f, (size_t)B * w.T[6] * kD * 4, hipMemcpyDeviceToDevice, s));
  return 0;
}

__global__ void f32_to_half_kernel(const float* in, uint16_t* out, size_t n, int is_bf16) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    if (is_bf16) {
      __bf16 v = (__bf16)in[i];
      memcpy(&out[i], &v, 2);
    } else {
      _Float16 v = (_Float16)in[i];
      memcpy(&out[i], &v, 2);
    }
  }
}

extern "C" int afx_head_forward(afx_handle h, const float* feats, int B, int T, float* logits, void* ws,
                                size_t ws_bytes, void* stream) {
  if (check_call(h, feats, B, T, logits, ws)) return 1;
  if (h->cfg.arch == AFX_ARCH_SSL) return fail("afx_head_forward: this handle has no back-end");
  if (h->cfg.arch == AFX_ARCH_CONFORMER_HEAD) return fail("afx_head_forward: this handle holds Conformer blocks only; use afx_conformer_forward");
  Ws w;
  memset(&w, 0, sizeof w);
  if (carve_ws("afx_head_forward", h, B, 0, T, ws, ws_bytes, &w)) return 1;
  hipStream_t s = (hipStream_t)stream;
  const size_t n = (size_t)B * T * kD;
  HIP_OK(hipMemcpyAsync(w.ssl_f, feats, n * 4, hipMemcpyDeviceToDevice, s));
  if (h->dt == AFX_DT_FP32) {
    HIP_OK(hipMemcpyAsync(w.ssl_h, feats, n * 4, hipMemcpyDeviceToDevice, s));
  } else {
    hipLaunchKernelGGL(f32_to_half_kernel, dim3(1024), dim3(256), 0, s, feats, (uint16_t*)w.ssl_h, n,
                       h->dt == AFX_DT_BF16 ? 1 : 0);
    HIP_OK(hipGetLastError());
  }
  Call cx(h, stream, w);
  return run_head(cx, B, T, w, logits);
}

// MyConformer.forward alone (models/conformer_baseline.py:22-29): tokens (B,T,emb) fp32 -> class token prepended -> the
// Conformer blocks -> logits (B,2) = fc5(token 0), embedding (B,emb) = token 0.  Workspace: afx_head_workspace_bytes(h, B, T).
extern "C" int afx_conformer_forward(afx_handle h, const float* tokens, int B, int T, float* logits, float* embedding,
                                     void* ws, size_t ws_bytes, void* stream) {
  if (check_call(h, tokens, B, T, logits, ws)) return 1;
  if (h->cfg.arch != AFX_ARCH_CONFORMER && h->cfg.arch != AFX_ARCH_CONFORMER_HEAD)
    return fail("afx_conformer_forward: this handle holds no Conformer blocks");
  Ws w;
  memset(&w, 0, sizeof w);
  if (carve_ws("afx_conformer_forward", h, B, 0, T, ws, ws_bytes, &w)) return 1;
  Call cx(h, stream, w);
  return run_conformer(cx, B, T, w, logits, tokens, embedding);
}

extern "C" size_t afx_head_workspace_bytes(afx_handle h, int B, int T) {
  if (!h || B <= 0 || T <= 0) return 0;
  Ws w;
  memset(&w, 0, sizeof w);
  return carve(h, B, 0, T, nullptr, &w);
}

// ---------------------------------------------------------------------------------
// single-kernel entry points
// ---------------------------------------------------------------------------------
extern "C" int afx_k_gemm(int dtype, const void* A, long lda, const void* W, long ldw, int M, int N, int K,
                          const float* bias, int act, float alpha, const float* resid, long ldr, float* out_f,
                          long ldo_f, void* out_h, long ldo_h, void* stream) {
  GemmArgs g = plain_gemm(A, lda, W, ldw, M, N, K);
  g.bias = bias; g.act = act; g.alpha = alpha; g.resid = resid; g.ldr = ldr;
  g.out_f = out_f; g.ldo_f = ldo_f; g.out_h = out_h; g.ldo_h = ldo_h;
  if (dtype == DT_FP16X3) {
    // Test hook of the split-precision product: A (M,K) and W (N,K) are FP32 here; the operand forms the engine keeps
    // (weight rows [hi | lo] + row scales, built once per checkpoint; the A planes, built per product in the workspace)
    // are built per call in temporary device memory, and the call synchronises the stream before it frees them.
    hipStream_t s = (hipStream_t)stream;
    if (K % 32 || lda != K || ldw != K || ((size_t)A & 15)) return fail("afx_k_gemm(fp16x3): contiguous 16-byte aligned rows, K %% 32 == 0");
    void *wp = nullptr, *planes = nullptr;
    const long span = ((long)M * K + 31) & ~31L;
    if (hipMalloc(&wp, (size_t)N * K * 4 + (size_t)N * 4) != hipSuccess || hipMalloc(&planes, (size_t)span * 4) != hipSuccess) {
      (void)hipFree(wp);
      return fail("afx_k_gemm(fp16x3): device allocation failed");
    }
    float* sc = (float*)((char*)wp + (size_t)N * K * 4);
    const char* m = launch_pack_linear((const float*)W, N, K, K, wp, DT_FP32, s);
    if (!m) m = launch_split_weight_rows(wp, N, K, sc, s);
    if (!m) m = launch_split_pairs((const float*)A, span, planes, kS3ScaleFree, s);
    if (!m) {
      g.A = planes; g.W = wp; g.k1 = K; g.K = 2 * K; g.kchunk = 2 * K; g.a_row = 2L * K; g.ldw = 2L * K; g.pre_scale = sc; g.a_inv = 1.0f / kS3ScaleFree;
      m = launch_gemm(g, DT_FP16X3, 1, s);
    }
    (void)hipStreamSynchronize(s);
    (void)hipFree(wp);
    (void)hipFree(planes);
    return m ? fail("%s", m) : 0;
  }
  KRET(launch_gemm(g, dtype, 1, (hipStream_t)stream));
}
extern "C" int afx_k_conv_gemm(int dtype, const void* in_h, const void* Wp, int B, int Tin, int Tout, int Cin, int k,
                               int s_, int N, const float* bias, float* out_f, void* stream) {
  GemmArgs g = plain_gemm(in_h, 0, Wp, (long)k * Cin, B * Tout, N, k * Cin);
  g.rpb = Tout; g.a_batch = (long)Tin * Cin; g.a_row = (long)s_ * Cin;
  g.o_batch_rows = Tout; g.oh_batch_rows = Tout;
  g.bias = bias; g.out_f = out_f; g.ldo_f = N;
  KRET(launch_gemm(g, dtype, 1, (hipStream_t)stream));
}
extern "C" int afx_k_conv_ln_act(int dtype, const void* in_h, const void* Wp, int B, int Tin, int Tout, int Cin,
                                 int k, int s_, const float* bias, const float* gamma, const float* beta, float eps,
                                 int act, float* out_f, void* out_h, void* stream) {
  GemmArgs g = plain_gemm(in_h, 0, Wp, (long)k * Cin, B * Tout, 512, k * Cin);
  g.rpb = Tout; g.a_batch = (long)Tin * Cin; g.a_row = (long)s_ * Cin;
  g.o_batch_rows = Tout; g.oh_batch_rows = Tout;
  g.bias = bias; g.act = act; g.ln_gamma = gamma; g.ln_beta = beta; g.ln_eps = eps;
  g.out_f = out_f; g.ldo_f = 512; g.out_h = out_h; g.ldo_h = 512;
  KRET(launch_gemm(g, dtype, 1, (hipStream_t)stream));
}
extern "C" int afx_k_pack_linear(int dtype, const float* w, int N, int K, int Kpad, void* out_h, void* stream) {
  KRET(launch_pack_linear(w, N, K, Kpad, out_h, dtype, (hipStream_t)stream));
}
extern "C" int afx_k_pack_conv(int dtype, const float* w, int N, int Cin, int k, void* out_h, void* stream) {
  KRET(launch_pack_conv(w, N, Cin, k, out_h, dtype, (hipStream_t)stream));
}
extern "C" size_t afx_k_conv0_pack_bytes(void) { return conv0_pack_bytes(); }
extern "C" int afx_k_conv0_pack(const float* w, const float* bias, void* pack, void* stream) {
  if (!w || !bias || !pack) return fail("afx_k_conv0_pack: null argument");
  KRET(launch_conv0_pack(w, bias, pack, (hipStream_t)stream));
}
// pack: the layer's split-precision operand block (afx_k_conv0_pack, built ONCE per checkpoint); asynchronous, allocates nothing
extern "C" int afx_k_conv0_packed(int dtype, const float* wave, int B, int L, const void* pack, const float* w,
                                  const float* bias, const float* gamma, const float* beta, int pre_emph, float coef,
                                  void* out_h, void* stream) {
  if (dtype != DT_FP32 && !pack) return fail("afx_k_conv0_packed: null pack");
  KRET(launch_conv0(wave, B, L, (L - 10) / 5 + 1, w, bias, gamma, beta, pre_emph, coef, out_h, dtype, (hipStream_t)stream,
                    dtype != DT_FP32 ? pack : nullptr));
}
// (test hook of round 1: builds the pack per call -- a device allocation and a stream synchronisation; hot paths use
// afx_k_conv0_pack once + afx_k_conv0_packed)
extern "C" int afx_k_conv0(int dtype, const float* wave, int B, int L, const float* w, const float* bias,
                           const float* gamma, const float* beta, int pre_emph, float coef, void* out_h,
                           void* stream) {
  void* pack = nullptr;
  if (dtype != DT_FP32) {
    if (hipMalloc(&pack, conv0_pack_bytes()) != hipSuccess) return fail("afx_k_conv0: device allocation failed");
    if (const char* m = launch_conv0_pack(w, bias, pack, (hipStream_t)stream)) {
      (void)hipFree(pack);
      return fail("%s", m);
    }
  }
  const char* m = launch_conv0(wave, B, L, (L - 10) / 5 + 1, w, bias, gamma, beta, pre_emph, coef, out_h, dtype,
                               (hipStream_t)stream, pack);
  if (pack) {
    (void)hipStreamSynchronize((hipStream_t)stream);
    (void)hipFree(pack);
  }
  if (m) return fail("%s", m);
  return 0;
}
extern "C" int afx_debug_set(const char* key, int value) {
  if (!key) return fail("afx_debug_set: null key");
  if (!strcmp(key, "gemm_map")) {
    gemm_set_map_mode(value);
    return 0;
  }
  if (!strcmp(key, "aasist_stop")) {
    aasist_set_stop(value);
    return 0;
  }
  if (!strcmp(key, "aasist_conv_slots")) {
    aasist_set_conv_slots(value);
    return 0;
  }
  if (!strcmp(key, "gemm_tile")) {
    gemm_set_tile(value);
    return 0;
  }
  if (!strcmp(key, "gemm_small_deep")) {
    gemm_set_small_deep(value);
    return 0;
  }
  if (!strcmp(key, "gemm_s3_small")) {
    gemm_set_s3_small(value);
    return 0;
  }
  if (!strcmp(key, "gemm_split")) {
    gemm_set_split(value);
    return 0;
  }
  if (!strcmp(key, "gemm_conv_split")) {
    gemm_set_conv_split(value);
    return 0;
  }
  if (!strcmp(key, "gemm_ph4")) {
    gemm_set_ph4(value);
    return 0;
  }
  if (!strcmp(key, "gemm_fit")) {
    gemm_set_fit(value);
    return 0;
  }
  if (!strcmp(key, "dispatch_objective")) {
    dispatch_force_objective(value);
    return 0;
  }
  if (!strcmp(key, "dispatch_cu_mask")) {
    dispatch_set_cu_mask(value);
    return 0;
  }
  if (!strcmp(key, "conf_chain_waves")) {
    conf_chain_set_waves(value);
    return 0;
  }
  if (!strcmp(key, "conf_attn_waves")) {
    conf_attn_mfma_set_waves(value);
    return 0;
  }
  if (!strcmp(key, "mhsa_vtr")) {
    mhsa_set_vtr(value);
    return 0;
  }
  if (!strcmp(key, "mhsa_zsplit")) {
    mhsa_set_zsplit(value);
    return 0;
  }
  if (!strcmp(key, "mhsa_waves")) {
    mhsa_set_waves(value);
    return 0;
  }
  if (!strcmp(key, "mhsa_force_long")) {
    mhsa_set_force_long(value);
    return 0;
  }
  if (!strcmp(key, "conf_attn_force_long")) {
    conf_attn_mfma_set_force_long(value);
    return 0;
  }
  if (!strcmp(key, "conf_attn_block")) {
    conf_attn_set_block(value);
    return 0;
  }
  if (!strcmp(key, "gemm_deep")) {
    gemm_set_deep(value);
    return 0;
  }
  if (!strcmp(key, "gemm_nodma")) {
    if (!gemm_set_nodma(value)) return fail("afx_debug_set: gemm_nodma exists only in the attribution build (make attr, AFX_LIB=.../libafx_attr.so)");
    return 0;
  }
  if (!strcmp(key, "gemm_a_nt")) {
    gemm_set_a_nt(value);
    return 0;
  }
  if (!strcmp(key, "conv0_mfma")) {
    conv0_set_mfma(value);
    return 0;
  }

  return fail("afx_debug_set: unknown key '%s'", key);
}
extern "C" int afx_engine_set(afx_handle h, const char* key, int value) {
  if (!h || !key) return fail("afx_engine_set: null argument");
  if (!strcmp(key, "posconv_sliding")) h->posconv_sliding = value != 0;
  else if (!strcmp(key, "conf_attn_mfma")) h->conf_attn_mfma = value != 0;
  else if (!strcmp(key, "fuse_conformer")) h->fuse_conformer = value != 0;
  else if (!strcmp(key, "fuse_conv_ln")) h->fuse_conv_ln = value != 0;
  else if (!strcmp(key, "gemm_small_deep")) h->gemm_small_deep = value != 0;
  else if (!strcmp(key, "concurrent")) h->concurrent = value != 0;
  else return fail("afx_engine_set: unknown key '%s'", key);
  return 0;
}
extern "C" int afx_engine_get(afx_handle h, const char* key, int* value) {
  if (!h || !key || !value) return fail("afx_engine_get: null argument");
  if (!strcmp(key, "concurrent")) *value = h->concurrent;
  else if (!strcmp(key, "objective")) *value = h->last_objective;
  else return fail("afx_engine_get: unknown key '%s'", key);
  return 0;
}
// The launch plan of a product, from host arithmetic alone (no device, no handle): what launch_gemm would do with it.
// flags: 1 fused LayerNorm epilogue (the conv layers), 2 split precision (K counts fp32 elements), 4 an activation outside the
// lean epilogue (swish / selu), 8 never the deep 128x64 tile.  objective: 0 makespan, 1 CU time, -1 what a launch outside any
// forward gets (the forced "dispatch_objective" knob when it is set, else makespan).
// out[8]: family, instance, tile rows, tile slots, split rows, remainder instance, remainder tile slots, objective used.
extern "C" int afx_gemm_plan(int M, int N, int K, int rpb, int kchunk, int groups, int flags, int objective, int* out) {
  if (!out || M <= 0 || N <= 0 || K <= 0 || groups <= 0) return fail("afx_gemm_plan: bad arguments");
  GemmArgs g = plain_gemm(nullptr, K, nullptr, K, M, N, K);
  if (rpb > 0) g.rpb = rpb;
  if (kchunk > 0) g.kchunk = kchunk;
  if (flags & 1) g.ln_gamma = g.ln_beta = g.bias = (const float*)out;  // (never dereferenced: the plan reads shapes only)
  if (flags & 2) { g.k1 = K; g.K = 2 * K; g.kchunk = 2 * g.kchunk; }
  if (flags & 4) g.act = ACT_SWISH;
  if (flags & 8) g.no_deep = 1;
  const int obj = objective < 0 ? dispatch_objective(OBJ_MAKESPAN) : (objective ? OBJ_CU_TIME : OBJ_MAKESPAN);
  const GemmPlan pl = gemm_plan(g, groups, obj);
  out[0] = pl.family; out[1] = pl.tile; out[2] = pl.rows; out[3] = (int)pl.tiles;
  out[4] = pl.split_rows; out[5] = pl.rem_tile; out[6] = (int)pl.rem_tiles; out[7] = obj;
  return 0;
}
extern "C" int afx_conf_chain_waves(int M, int objective) {
  return conf_chain_waves_of(M, objective < 0 ? dispatch_objective(OBJ_MAKESPAN) : (objective ? OBJ_CU_TIME : OBJ_MAKESPAN));
}
extern "C" int afx_k_pre_emphasis(const float* x, int B, int L, float coef, float* y, void* stream) {
  KRET(launch_pre_emphasis(x, B, L, coef, y, (hipStream_t)stream));
}
extern "C" int afx_k_tile_crop(const float* x, const long long* offs, const long long* starts, int B, int duration,
                               float* out, void* stream) {
  if (!x || !offs || !out) return fail("afx_k_tile_crop: null argument");
  KRET(launch_tile_crop(x, offs, starts, B, duration, out, (hipStream_t)stream));
}
extern "C" int afx_k_rownorm(int dtype, const float* x, long ldx, int rows, int C, const float* gamma,
                             const float* beta, float eps, int act, float* out_f, long ldo_f, void* out_h, long ldo_h,
                             void* stream) {
  RowNormArgs a = plain_norm(x, ldx, rows, C);
  a.gamma = gamma; a.beta = beta; a.eps = eps; a.act = act; a.out_f = out_f; a.ldo_f = ldo_f; a.out_h = out_h; a.ldo_h = ldo_h;
  KRET(launch_rownorm(a, dtype, (hipStream_t)stream));
}
extern "C" int afx_k_mhsa(int dtype, const void* qkv, void* out, int B, int T, int H, void* stream) {
  if (dtype == DT_FP16X3) KRET(launch_mhsa_split((const float*)qkv, (float*)out, B, T, H, (hipStream_t)stream));  // fp32 rows in / out
  KRET(launch_mhsa(qkv, out, B, T, H, dtype, (hipStream_t)stream));
}
extern "C" int afx_k_conf_attn(int dtype, const float* q, long ldq, const float* kv, long ldkv, const float* rel,
                               int max_pos, int B, int N, int H, int dh, void* out_h, long ldo, void* stream) {
  KRET(launch_conf_attn(q, ldq, kv, ldkv, rel, max_pos, B, N, H, dh, out_h, ldo, dtype, (hipStream_t)stream));
}
extern "C" int afx_k_conf_attn_mfma(int dtype, const float* q, long ldq, const float* kv, long ldkv, const void* rel_h,
                                    int max_pos, int B, int N, int H, int dh, void* out_h, long ldo, void* stream) {
  if (dtype == DT_FP16X3)  // split precision: fp32 rows out, the table as fp32 rows padded to 64 (afx_k_pack_linear with dtype fp32)
    KRET(launch_conf_attn_split(q, ldq, kv, ldkv, (const float*)rel_h, max_pos, B, N, H, dh, (float*)out_h, ldo, (hipStream_t)stream));
  KRET(launch_conf_attn_mfma(q, ldq, kv, ldkv, rel_h, max_pos, B, N, H, dh, out_h, ldo, dtype, (hipStream_t)stream));
}
extern "C" int afx_k_conf_dwconv(int dtype, const float* x, long ldx, const float* w, const float* bias,
                                 const float* bn_scale, const float* bn_shift, int B, int N, int C, int k, void* out_h,
                                 long ldo, void* stream) {
  KRET(launch_conf_dwconv(x, ldx, w, bias, bn_scale, bn_shift, B, N, C, k, out_h, ldo, dtype, (hipStream_t)stream));
}
