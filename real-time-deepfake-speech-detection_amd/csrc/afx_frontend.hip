// Frontend / row kernels for gfx950: raw-waveform conv layer 0 with fused
// LayerNorm + GELU, generic row LayerNorm, weight packing.
#include <type_traits>

#include "afx_common.h"
#include "afx_kernels.h"

namespace afx {

// ---------------------------------------------------------------------------------
// conv layer 0: Conv1d(1 -> 512, k=10, s=5, bias) ->
// LayerNorm over the 512 channels (fp32 statistics) -> erf-GELU -> operand type.
// HBM-bound by its 1-KB-per-frame output (256 KB of waveform in, 13 MB out per 4-s
// utterance).  One WAVE per frame: lane l owns channels 8l..8l+7 (weights, bias,
// gamma, beta resident in VGPRs for the whole block), the 10 input samples are LDS
// broadcasts, LayerNorm statistics are two 64-lane shuffle reductions, and the wave
// stores one contiguous 1-KB row (16 B per lane).  Optional pre-emphasis
// (data/preprocess.py:16-29) is applied while the waveform window is staged in LDS.
// ---------------------------------------------------------------------------------
constexpr int C0_FB = 64;  // frames per workgroup
static int g_conv0_mfma = 1;  // A/B knob: 1 = matrix-core forms of conv layer 0 (split-precision fp16 with a packed operand, else fp32 MFMA), 2 = fp32 MFMA always, 0 = the VALU form below

template <class HT>
__global__ __launch_bounds__(256) void conv0_kernel(const float* __restrict__ wave, int L, int T0,
                                                    const float* __restrict__ w, const float* __restrict__ bias,
                                                    const float* __restrict__ gamma, const float* __restrict__ beta,
                                                    int pre_emph, float pre_coef, typename HT::T* __restrict__ out) {
  typedef typename HT::T T;
  typedef typename HT::V8 V8;
  __shared__ float xs[C0_FB * 5 + 8];
  const int b = blockIdx.y;
  const int f0 = blockIdx.x * C0_FB;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const float* x = wave + (long)b * L;
  const int s0 = f0 * 5;
  for (int i = tid; i < C0_FB * 5 + 5; i += 256) {
    const int gidx = s0 + i;
    float v = 0.f;
    if (gidx < L) {
      v = x[gidx];
      if (pre_emph) {
        const int gp = gidx > 0 ? gidx - 1 : 1;  // reflect pad of one sample on the left
        v -= pre_coef * x[gp];
      }
    }
    xs[i] = v;
  }
  float wr[8][10], bi[8], ga[8], be[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = lane * 8 + i;
#pragma unroll
    for (int j = 0; j < 10; ++j) wr[i][j] = w[c * 10 + j];
    bi[i] = bias[c];
    ga[i] = gamma[c];
    be[i] = beta[c];
  }
  __syncthreads();
  const int fend = min(C0_FB, T0 - f0);
  for (int f = wv; f < fend; f += 4) {
    float xv[10];
#pragma unroll
    for (int j = 0; j < 10; ++j) xv[j] = xs[f * 5 + j];
    float v[8];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      float a = bi[i];
#pragma unroll
      for (int j = 0; j < 10; ++j) {
        a = fmaf(wr[i][j], xv[j], a);
        scalar_only(a);
      }
      v[i] = a;
      sum += a;
    }
#ifdef AFX_C0_KEEPX  // diagnostics only (with AFX_C0_PACKED): the samples stay live past the loop, so the packed loop cannot write
#pragma unroll       // an accumulator over the sample pair it reads -- packed math WITHOUT the in-place cross-half form
    for (int j = 0; j < 10; ++j) asm volatile("" ::"v"(xv[j]), "v"(sum));  // (after the last accumulation: it needs `sum`)
#endif
    const float mean = wave_sum(sum) * (1.0f / 512.0f);
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      v[i] -= mean;
      sq = fmaf(v[i], v[i], sq);
    }
    const float rstd = 1.0f / sqrtf(wave_sum(sq) * (1.0f / 512.0f) + 1e-5f);
    V8 o;
#pragma unroll
    for (int i = 0; i < 8; i += 2) {  // two channels per packed-math GELU
      const f32x2_t yin = f32x2_t{fmaf(v[i] * rstd, ga[i], be[i]), fmaf(v[i + 1] * rstd, ga[i + 1], be[i + 1])};
      const f32x2_t y = sizeof(T) == 4 ? gelu_erf2(yin) : gelu_poly2(yin);  // fp32 = exact mode
      o[i] = (T)y[0];
      o[i + 1] = (T)y[1];
    }
    *(V8*)(out + ((long)b * T0 + f0 + f) * 512 + lane * 8) = o;
  }
}

// The same layer with the 10-tap products on the fp32 matrix instruction (exact fp32, like the VALU
// form above): out^T tile = W (16 channels x 12 taps, zero padded) . frames (12 x 16), three
// v_mfma_f32_16x16x4_f32 per 16-channel tile.  A lane then holds 4 consecutive channels x 32 tiles
// of ONE frame: the LayerNorm statistics are a 4-lane reduction per 16 frames (not a 64-lane one per
// frame), and only LayerNorm + GELU + convert remain on the VALU: ~80 instructions per frame instead
// of ~185.  Workgroup = 256 frames (4 waves x 4 groups of 16); weights (24 KB, tap-padded) and the
// waveform window live in LDS.
#ifndef CONV0_DBG
#define CONV0_DBG 0  // timing experiments only (wrong results): 1 no GELU, 2 no stores, 4 no MFMA, 8 no LayerNorm statistics
#endif
constexpr int C0M_FB = 256;
template <class HT>
__global__ __launch_bounds__(256, 2) void conv0_mfma_kernel(const float* __restrict__ wave, int L, int T0,
                                                         const float* __restrict__ w, const float* __restrict__ bias,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         int pre_emph, float pre_coef, typename HT::T* __restrict__ out) {
  typedef typename HT::T T;
  typedef typename HT::V8 V8;
  __shared__ float xs[C0M_FB * 5 + 16];
  __shared__ float ws[3 * 32 * 64];      // [k-step][channel tile][lane]: the lane's A-operand value
  __shared__ float pv[3 * 512];          // bias | gamma | beta
  const int b = blockIdx.y, f0 = blockIdx.x * C0M_FB;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const float* x = wave + (long)b * L;
  const int s0 = f0 * 5;
  for (int i = tid; i < C0M_FB * 5 + 16; i += 256) {
    const int gidx = s0 + i;
    float v = 0.f;
    if (gidx < L) {
      v = x[gidx];
      if (pre_emph) {
        const int gp = gidx > 0 ? gidx - 1 : 1;  // reflect pad of one sample on the left
        v -= pre_coef * x[gp];
      }
    }
    xs[i] = v;
  }
  for (int i = tid; i < 3 * 32 * 64; i += 256) {
    const int s = i / 2048, ct = (i >> 6) & 31, l = i & 63;
    const int tap = 4 * s + (l >> 4);
    ws[i] = tap < 10 ? w[(ct * 16 + (l & 15)) * 10 + tap] : 0.f;
  }
  for (int i = tid; i < 512; i += 256) {
    pv[i] = bias[i];
    pv[512 + i] = gamma[i];
    pv[1024 + i] = beta[i];
  }
  __syncthreads();
  const int fr = lane & 15, kq = lane >> 4;
  for (int grp = 0; grp < 4; ++grp) {
    const int fl = (wv * 4 + grp) * 16;  // first frame of this group inside the workgroup
    if (f0 + fl >= T0) break;
    float bx[3];
#pragma unroll
    for (int s = 0; s < 3; ++s) bx[s] = xs[(fl + fr) * 5 + 4 * s + kq];
    f32x4 acc[32];
#pragma unroll
    for (int ct = 0; ct < 32; ++ct) {
      f32x4 c = *(const f32x4*)(pv + ct * 16 + kq * 4);  // bias: the accumulator's own channels
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        if constexpr ((CONV0_DBG & 4) != 0) c[0] += ws[(s * 32 + ct) * 64 + lane] * bx[s];
        else c = __builtin_amdgcn_mfma_f32_16x16x4f32(ws[(s * 32 + ct) * 64 + lane], bx[s], c, 0, 0, 0);
      }
      acc[ct] = c;
    }
    float sum = 0.f;
#pragma unroll
    for (int ct = 0; ct < 32; ++ct) sum += (acc[ct][0] + acc[ct][1]) + (acc[ct][2] + acc[ct][3]);
    const float mean = rows_sum(sum) * (1.0f / 512.0f);
    float sq = 0.f;
#pragma unroll
    for (int ct = 0; ct < 32; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        acc[ct][r] -= mean;
        sq = fmaf(acc[ct][r], acc[ct][r], sq);
      }
    const float rstd = 1.0f / sqrtf(rows_sum(sq) * (1.0f / 512.0f) + 1e-5f);
    const int f = f0 + fl + fr;
    T* orow = out + ((long)b * T0 + (f < T0 ? f : T0 - 1)) * 512;
    const int cb = (kq & 1) * 16 + (kq >> 1) * 8;
#pragma unroll
    for (int cp = 0; cp < 16; ++cp) {  // channel-tile pairs -> 8 consecutive channels per lane
      f32x4 va, vb;
      {
        const f32x4 g0 = *(const f32x4*)(pv + 512 + cp * 32 + kq * 4), b0 = *(const f32x4*)(pv + 1024 + cp * 32 + kq * 4);
        const f32x4 g1 = *(const f32x4*)(pv + 512 + cp * 32 + 16 + kq * 4), b1 = *(const f32x4*)(pv + 1024 + cp * 32 + 16 + kq * 4);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          va[r] = fmaf(acc[2 * cp][r] * rstd, g0[r], b0[r]);
          vb[r] = fmaf(acc[2 * cp + 1][r] * rstd, g1[r], b1[r]);
        }
        if constexpr ((CONV0_DBG & 1) == 0) gelu_poly8(va, vb);  // all 8 values step by step together
      }
      V8 h;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(va[r]), __float_as_uint(vb[r]), false, false);
        h[r] = (T)__uint_as_float(sw[0]);
        h[4 + r] = (T)__uint_as_float(sw[1]);
      }
      if constexpr ((CONV0_DBG & 2) != 0) asm volatile("" :: "v"(h));
      else if (f < T0) *(V8*)(orow + cp * 32 + cb) = h;
    }
  }
}

// ---------------------------------------------------------------------------------
// conv layer 0 at fp32 accuracy on the fp16 matrix pipe (the half-precision engines' form): the 10 taps, their
// split-precision corrections and the bias are ONE v_mfma_f32_16x16x32_f16 per 16 channels x 16 frames instead of
// three v_mfma_f32_16x16x4_f32 (16 against 96 matrix-pipe cycles):
//     k  0.. 9  xh[tap] * wh[tap]          x = xh + xl, w = wh + wl (fp16 hi + fp16 lo of the remainder)
//     k 10..19  xl[tap] * wh[tap]
//     k 20..29  xh[tap] * wl[tap]          (xl * wl, 2^-22 relative, is dropped)
//     k 30, 31  (G / cb) * (cb bias)_hi, (G / cb) * (cb bias)_lo      (cb: power of two, largest |bias| into [1, 2))
// Each frame is scaled by a power of two S_f that brings its largest sample into [1, 2) and the weights by one power of
// two c for the layer (largest |w| into [1, 2)), so that the lo parts sit in fp16's normal range whatever the recording
// level; G = S_f * c multiplies the whole pre-norm row and the LayerNorm that follows divides it out again
// (eps -> G^2 eps).  S_f depends on the frame's own 10 samples only: a frame's result does not depend on its
// neighbours, the batch or the launch (the streaming scorer relies on that).
// The packed weight operand (conv0_pack_kernel, once per checkpoint): [32 channel tiles][64 lanes][8 halfs] in MFMA
// A-operand order, followed by the exponents of c and cb.
// ---------------------------------------------------------------------------------
constexpr int C0P_HALFS = 32 * 64 * 8;
__global__ __launch_bounds__(256) void conv0_pack_kernel(const float* __restrict__ w, const float* __restrict__ bias,
                                                         _Float16* __restrict__ pack) {
  __shared__ float red[256];
  const int tid = threadIdx.x;
  auto norm_exp = [&](const float* v, int n) {  // e with max|v| * 2^e in [1, 2), clamped to +-12
    float m = 0.f;
    for (int i = tid; i < n; i += 256) m = fmaxf(m, fabsf(v[i]));
    __syncthreads();
    red[tid] = m;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
      if (tid < st) red[tid] = fmaxf(red[tid], red[tid + st]);
      __syncthreads();
    }
    const float mx = red[0];
    int e = 0;
    if (mx > 0.f && mx < INFINITY) e = 127 - (int)((__float_as_uint(mx) >> 23) & 0xff);
    return e < -12 ? -12 : (e > 12 ? 12 : e);
  };
  const int cexp = norm_exp(w, 512 * 10), bexp = norm_exp(bias, 512);
  const float c = ldexpf(1.0f, cexp), cb = ldexpf(1.0f, bexp);
  for (int i = tid; i < 32 * 64; i += 256) {
    const int ct = i >> 6, l = i & 63, ch = ct * 16 + (l & 15), kg = l >> 4;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = kg * 8 + j;
      float v;
      if (k < 30) {
        const float wv = w[ch * 10 + (k < 10 ? k : (k < 20 ? k - 10 : k - 20))] * c;
        const float hi = (float)(_Float16)wv;
        v = k < 20 ? hi : wv - hi;
      } else {
        const float bv = bias[ch] * cb;
        const float hi = (float)(_Float16)bv;
        v = k == 30 ? hi : bv - hi;
      }
      pack[i * 8 + j] = (_Float16)v;
    }
  }
  if (tid == 0) {
    ((int*)(pack + C0P_HALFS))[0] = cexp;
    ((int*)(pack + C0P_HALFS))[1] = bexp;
  }
}

// HT = F32T (round 4): the split-precision engines ("fp16x3") run this kernel too -- its products are hi / lo fp16 pairs already --
// with the fp32-accurate erf-GELU and fp32 rows out, or, pair_scale > 0, the rows leave as conv layer 1's PAIR-FORM operand
// (afx_kernels.h) scaled by that power of two: no fp32 round trip and no split launch over the stack's largest activation.
template <class HT>
__global__ __launch_bounds__(256, 2) void conv0_split_kernel(const float* __restrict__ wave, int L, int T0,
                                                          const _Float16* __restrict__ pack, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, int pre_emph, float pre_coef,
                                                          typename HT::T* __restrict__ out, float pair_scale) {
  typedef typename HT::T T;
  typedef typename HT::V8 V8;
  constexpr bool F32 = std::is_same<T, float>::value;
  __shared__ float xs[C0M_FB * 5 + 16];
  __shared__ __attribute__((aligned(16))) _Float16 xop[C0M_FB * 32];  // per frame: the 32 k-values of its B operand
  __shared__ float Gs[C0M_FB];
  __shared__ __attribute__((aligned(16))) _Float16 wsh[C0P_HALFS];
  __shared__ float pv[2 * 512];  // gamma | beta
  const int b = blockIdx.y, f0 = blockIdx.x * C0M_FB;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const float* x = wave + (long)b * L;
  const int s0 = f0 * 5;
  for (int i = tid; i < C0M_FB * 5 + 16; i += 256) {
    const int gidx = s0 + i;
    float v = 0.f;
    if (gidx < L) {
      v = x[gidx];
      if (pre_emph) {
        const int gp = gidx > 0 ? gidx - 1 : 1;  // reflect pad of one sample on the left
        v -= pre_coef * x[gp];
      }
    }
    xs[i] = v;
  }
  for (int i = tid; i < C0P_HALFS / 8; i += 256) ((uint4*)wsh)[i] = ((const uint4*)pack)[i];
  const int cexp = ((const int*)(pack + C0P_HALFS))[0], bexp = ((const int*)(pack + C0P_HALFS))[1];
  for (int i = tid; i < 512; i += 256) {
    pv[i] = gamma[i];
    pv[512 + i] = beta[i];
  }
  __syncthreads();
  {  // thread = frame: scale, split, lay out the 32 k-values
    float xv[10], m = 0.f;
#pragma unroll
    for (int j = 0; j < 10; ++j) {
      xv[j] = xs[tid * 5 + j];
      m = fmaxf(m, fabsf(xv[j]));
    }
    const int eb = (int)((__float_as_uint(m) >> 23) & 0xff);
    int ge = (eb > 0 && eb < 255 ? 127 - eb : 0) + cexp;  // exponent of G = S_f * c; S_f * m in [1, 2)
    int qe = ge - bexp;                                   // G / cb is an fp16 operand (k = 30, 31): keep it normal
    qe = qe < -14 ? -14 : (qe > 15 ? 15 : qe);
    ge = qe + bexp;
    // a frame far beyond any audio scale (|x| > 2^14 / its scale): keep S_f * m inside fp16 and let the bias operand
    // underflow instead -- against such a signal the bias is below fp32 resolution anyway
    if (eb > 0 && eb < 255 && ge - cexp + (eb - 127) > 14) {
      ge = 14 - (eb - 127) + cexp;
      qe = ge - bexp;
    }
    const float S = ldexpf(1.0f, ge - cexp), G = ldexpf(1.0f, ge);
    _Float16 h[32];
#pragma unroll
    for (int j = 0; j < 10; ++j) {
      const float v = xv[j] * S;
      const _Float16 hi = (_Float16)v;
      h[j] = hi;
      h[10 + j] = (_Float16)(v - (float)hi);
      h[20 + j] = hi;
    }
    h[30] = h[31] = (_Float16)ldexpf(1.0f, qe);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      f16x8 t;
#pragma unroll
      for (int j = 0; j < 8; ++j) t[j] = h[q * 8 + j];
      *(f16x8*)(xop + tid * 32 + q * 8) = t;
    }
    Gs[tid] = G;
  }
  __syncthreads();
  const int fr = lane & 15, kq = lane >> 4;
  for (int grp = 0; grp < 4; ++grp) {
    const int fl = (wv * 4 + grp) * 16;  // first frame of this group inside the workgroup
    if (f0 + fl >= T0) break;
    const f16x8 bx = *(const f16x8*)(xop + (fl + fr) * 32 + kq * 8);
    const float G = Gs[fl + fr];
    f32x4 acc[32];
#pragma unroll
    for (int ct = 0; ct < 32; ++ct)
      acc[ct] = FP16::mfma(*(const f16x8*)(wsh + (ct * 64 + lane) * 8), bx, f32x4{0.f, 0.f, 0.f, 0.f});
    float sum = 0.f;
#pragma unroll
    for (int ct = 0; ct < 32; ++ct) sum += (acc[ct][0] + acc[ct][1]) + (acc[ct][2] + acc[ct][3]);
    const float mean = rows_sum(sum) * (1.0f / 512.0f);
    float sq = 0.f;
#pragma unroll
    for (int ct = 0; ct < 32; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        acc[ct][r] -= mean;
        sq = fmaf(acc[ct][r], acc[ct][r], sq);
      }
    const float rstd = 1.0f / sqrtf(rows_sum(sq) * (1.0f / 512.0f) + (G * G) * 1e-5f);
    const int f = f0 + fl + fr;
    T* orow = out + ((long)b * T0 + (f < T0 ? f : T0 - 1)) * 512;
    const int cb = (kq & 1) * 16 + (kq >> 1) * 8;
#pragma unroll
    for (int cp = 0; cp < 16; ++cp) {  // channel-tile pairs -> 8 consecutive channels per lane
      f32x4 va, vb;
      {
        const f32x4 g0 = *(const f32x4*)(pv + cp * 32 + kq * 4), b0 = *(const f32x4*)(pv + 512 + cp * 32 + kq * 4);
        const f32x4 g1 = *(const f32x4*)(pv + cp * 32 + 16 + kq * 4), b1 = *(const f32x4*)(pv + 512 + cp * 32 + 16 + kq * 4);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          va[r] = fmaf(acc[2 * cp][r] * rstd, g0[r], b0[r]);
          vb[r] = fmaf(acc[2 * cp + 1][r] * rstd, g1[r], b1[r]);
        }
        if constexpr (F32) {  // fp32 results: the fp32-accurate erf form (the polynomial is sized for fp16 outputs)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            va[r] = gelu_erf(va[r]);
            vb[r] = gelu_erf(vb[r]);
          }
        } else {
          gelu_poly8(va, vb);
        }
      }
      float w8[8];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(va[r]), __float_as_uint(vb[r]), false, false);
        w8[r] = __uint_as_float(sw[0]);
        w8[4 + r] = __uint_as_float(sw[1]);
      }
      if (f >= T0) continue;
      if constexpr (F32) {
        if (pair_scale > 0.f) {  // columns cp * 32 + cb .. + 7 of the row's pair form: inside one 32-element group
          f16x8 hi, lo;
#pragma unroll
          for (int r = 0; r < 8; ++r) {
            const float sv = w8[r] * pair_scale;
            hi[r] = (_Float16)sv;
            lo[r] = (_Float16)(sv - (float)hi[r]);
          }
          _Float16* hp = (_Float16*)orow + cp * 64 + cb;
          *(f16x8*)hp = hi;
          *(f16x8*)(hp + 32) = lo;
          continue;
        }
      }
      V8 h;
#pragma unroll
      for (int r = 0; r < 8; ++r) h[r] = (T)w8[r];
      *(V8*)(orow + cp * 32 + cb) = h;
    }
  }
}

size_t conv0_pack_bytes() { return (size_t)C0P_HALFS * 2 + 16; }
const char* launch_conv0_pack(const float* w, const float* bias, void* pack, hipStream_t s) {
  if (!w || !bias || !pack) return "conv0_pack: null argument";
  hipLaunchKernelGGL(conv0_pack_kernel, dim3(1), dim3(256), 0, s, w, bias, (_Float16*)pack);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

// ---------------------------------------------------------------------------------
// conv layer 0 of the wav2vec2-*base* feature extractor (fairseq extractor_mode="default"; SURVEY 8a row 1a, the
// "GroupNorm/GELU" `north_star` names): bias-free Conv1d(1 -> 512, k=10, s=5) -> GroupNorm(512 groups of one channel
// = per (utterance, channel) normalisation over TIME, affine) -> erf-GELU.  The statistics span the whole clip, so
// the layer is two passes over the (cheap: 10 MACs per output) convolution: pass 1 writes per-chunk partial sums
// (sum, sum of squares) -- fixed chunks, summed in a fixed order in double by the finalize kernel, so the result does
// not depend on scheduling --, pass 2 recomputes the convolution, normalises, activates and stores.
// ---------------------------------------------------------------------------------
constexpr int GN_FB = 256;  // frames per statistics chunk
__global__ __launch_bounds__(256) void conv0_gn_stats_kernel(const float* __restrict__ wave, int L, int T0,
                                                             const float* __restrict__ w, float* __restrict__ part /*[B][nchunk][2][512]*/) {
  __shared__ float xs[GN_FB * 5 + 8];
  const int b = blockIdx.y, f0 = blockIdx.x * GN_FB, tid = threadIdx.x;
  const float* x = wave + (long)b * L;
  for (int i = tid; i < GN_FB * 5 + 5; i += 256) xs[i] = f0 * 5 + i < L ? x[f0 * 5 + i] : 0.f;
  float w0[10], w1[10];
#pragma unroll
  for (int j = 0; j < 10; ++j) {
    w0[j] = w[tid * 10 + j];
    w1[j] = w[(tid + 256) * 10 + j];
  }
  __syncthreads();
  const int nf = min(GN_FB, T0 - f0);
  float s0 = 0.f, q0 = 0.f, s1 = 0.f, q1 = 0.f;
  for (int f = 0; f < nf; ++f) {
    float a0 = 0.f, a1 = 0.f;
#pragma unroll
    for (int j = 0; j < 10; ++j) {
      const float xv = xs[f * 5 + j];
      a0 = fmaf(w0[j], xv, a0);
      a1 = fmaf(w1[j], xv, a1);
      scalar_only(a0);
      scalar_only(a1);
    }
    s0 += a0; q0 = fmaf(a0, a0, q0);
    s1 += a1; q1 = fmaf(a1, a1, q1);
  }
  float* o = part + ((long)b * gridDim.x + blockIdx.x) * 1024;
  o[tid] = s0; o[tid + 256] = s1; o[512 + tid] = q0; o[512 + tid + 256] = q1;
}
__global__ void conv0_gn_finalize_kernel(const float* __restrict__ part, int nchunk, int T0, float eps,
                                         float* __restrict__ mean, float* __restrict__ rstd) {
  const int b = blockIdx.x, c = threadIdx.x;  // 512 threads
  double s = 0.0, q = 0.0;
  for (int k = 0; k < nchunk; ++k) {
    const float* o = part + ((long)b * nchunk + k) * 1024;
    s += (double)o[c];
    q += (double)o[512 + c];
  }
  const double m = s / T0, v = q / T0 - m * m;
  mean[b * 512 + c] = (float)m;
  rstd[b * 512 + c] = (float)(1.0 / sqrt((v > 0.0 ? v : 0.0) + (double)eps));
}
template <class HT>
__global__ __launch_bounds__(256) void conv0_gn_apply_kernel(const float* __restrict__ wave, int L, int T0,
                                                             const float* __restrict__ w, const float* __restrict__ mean,
                                                             const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, typename HT::T* __restrict__ out) {
  typedef typename HT::T T;
  typedef typename HT::V8 V8;
  __shared__ float xs[C0_FB * 5 + 8];
  const int b = blockIdx.y, f0 = blockIdx.x * C0_FB;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const float* x = wave + (long)b * L;
  for (int i = tid; i < C0_FB * 5 + 5; i += 256) xs[i] = f0 * 5 + i < L ? x[f0 * 5 + i] : 0.f;
  float wr[8][10], sc[8], sh[8];  // lane owns channels 8 lane .. 8 lane + 7; y = conv * sc + sh
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = lane * 8 + i;
#pragma unroll
    for (int j = 0; j < 10; ++j) wr[i][j] = w[c * 10 + j];
    const float r = rstd[b * 512 + c] * gamma[c];
    sc[i] = r;
    sh[i] = fmaf(-mean[b * 512 + c], r, beta[c]);
  }
  __syncthreads();
  const int fend = min(C0_FB, T0 - f0);
  for (int f = wv; f < fend; f += 4) {
    float xv[10];
#pragma unroll
    for (int j = 0; j < 10; ++j) xv[j] = xs[f * 5 + j];
    V8 o;
#pragma unroll
    for (int i = 0; i < 8; i += 2) {
      float a0 = 0.f, a1 = 0.f;
#pragma unroll
      for (int j = 0; j < 10; ++j) {
        a0 = fmaf(wr[i][j], xv[j], a0);
        a1 = fmaf(wr[i + 1][j], xv[j], a1);
        scalar_only(a0);
        scalar_only(a1);
      }
      const f32x2_t yin = f32x2_t{fmaf(a0, sc[i], sh[i]), fmaf(a1, sc[i + 1], sh[i + 1])};
      const f32x2_t y = sizeof(T) == 4 ? gelu_erf2(yin) : gelu_poly2(yin);
      o[i] = (T)y[0];
      o[i + 1] = (T)y[1];
    }
    *(V8*)(out + ((long)b * T0 + f0 + f) * 512 + lane * 8) = o;
  }
}
const char* launch_conv0_groupnorm(const float* wave, int B, int L, int T0, const float* w, const float* gamma,
                                   const float* beta, float eps, float* stats /* B*(nchunk*1024 + 1024) floats */, void* out_h,
                                   int dtype, hipStream_t s) {
  if (B <= 0 || L < 10 || T0 != (L - 10) / 5 + 1 || B > 65535) return "conv0 (group norm): bad shape";
  const int nchunk = (T0 + GN_FB - 1) / GN_FB;
  float* part = stats;
  float* mean = stats + (size_t)B * nchunk * 1024;
  float* rstd = mean + (size_t)B * 512;
  hipLaunchKernelGGL(conv0_gn_stats_kernel, dim3(nchunk, B), dim3(256), 0, s, wave, L, T0, w, part);
  hipLaunchKernelGGL(conv0_gn_finalize_kernel, dim3(B), dim3(512), 0, s, part, nchunk, T0, eps, mean, rstd);
  dim3 grid((T0 + C0_FB - 1) / C0_FB, B);
  AFX_DISPATCH_HT(dtype, hipLaunchKernelGGL(conv0_gn_apply_kernel<HT>, grid, dim3(256), 0, s, wave, L, T0, w, mean, rstd, gamma,
                                            beta, (HT::T*)out_h));
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}
size_t conv0_groupnorm_stats_floats(int B, int T0) { return (size_t)B * (((size_t)T0 + GN_FB - 1) / GN_FB * 1024 + 1024); }

const char* launch_conv0(const float* wave, int B, int L, int T0, const float* w, const float* bias,
                         const float* gamma, const float* beta, int pre_emph, float pre_coef, void* out_h,
                         int dtype, hipStream_t s, const void* wpack, float pair_scale) {
  if (B <= 0 || L < 10 || T0 != (L - 10) / 5 + 1) return "conv0: bad shape";
  if (dtype == DT_FP16X3) {  // the split-precision engines: fp32 rows (or conv layer 1's pair-form operand) out
    if (!wpack) return "conv0 (fp16x3): the packed operand block is missing";
    dim3 grid((T0 + C0M_FB - 1) / C0M_FB, B);
    hipLaunchKernelGGL(conv0_split_kernel<F32T>, grid, dim3(256), 0, s, wave, L, T0, (const _Float16*)wpack, gamma, beta, pre_emph,
                       pre_coef, (float*)out_h, pair_scale);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? nullptr : hipGetErrorString(e);
  }
  if (dtype != DT_FP32 && g_conv0_mfma == 1 && wpack) {  // split precision on the fp16 matrix pipe (packed operand given)
    dim3 grid((T0 + C0M_FB - 1) / C0M_FB, B);
    if (dtype == DT_BF16)
      hipLaunchKernelGGL(conv0_split_kernel<BF16>, grid, dim3(256), 0, s, wave, L, T0, (const _Float16*)wpack, gamma, beta,
                         pre_emph, pre_coef, (__bf16*)out_h, 0.f);
    else
      hipLaunchKernelGGL(conv0_split_kernel<FP16>, grid, dim3(256), 0, s, wave, L, T0, (const _Float16*)wpack, gamma, beta,
                         pre_emph, pre_coef, (_Float16*)out_h, 0.f);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? nullptr : hipGetErrorString(e);
  }
  if (dtype != DT_FP32 && g_conv0_mfma) {
    dim3 grid((T0 + C0M_FB - 1) / C0M_FB, B);
    if (dtype == DT_BF16)
      hipLaunchKernelGGL(conv0_mfma_kernel<BF16>, grid, dim3(256), 0, s, wave, L, T0, w, bias, gamma, beta, pre_emph,
                         pre_coef, (__bf16*)out_h);
    else
      hipLaunchKernelGGL(conv0_mfma_kernel<FP16>, grid, dim3(256), 0, s, wave, L, T0, w, bias, gamma, beta, pre_emph,
                         pre_coef, (_Float16*)out_h);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? nullptr : hipGetErrorString(e);
  }
  dim3 grid((T0 + C0_FB - 1) / C0_FB, B);
  AFX_DISPATCH_HT(dtype, hipLaunchKernelGGL(conv0_kernel<HT>, grid, dim3(256), 0, s, wave, L, T0, w, bias, gamma, beta,
                                            pre_emph, pre_coef, (HT::T*)out_h));
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}
void conv0_set_mfma(int v) { g_conv0_mfma = v; }

// ---------------------------------------------------------------------------------
// Stand-alone pre-emphasis (data/preprocess.py:16-29) for callers that apply it as a
// separate module (trainer.py:104); the engine itself fuses it into conv0.
// ---------------------------------------------------------------------------------
__global__ void pre_emphasis_kernel(const float* __restrict__ x, int L, float coef, float* __restrict__ y) {
  const long base = (long)blockIdx.y * L;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < L; i += gridDim.x * blockDim.x) {
    const int p = i > 0 ? i - 1 : (L > 1 ? 1 : 0);  // reflect pad of one sample on the left
    y[base + i] = x[base + i] - coef * x[base + p];
  }
}
const char* launch_pre_emphasis(const float* x, int B, int L, float coef, float* y, hipStream_t s) {
  if (B <= 0 || L <= 0) return "pre_emphasis: empty input";
  hipLaunchKernelGGL(pre_emphasis_kernel, dim3(min((L + 255) / 256, 1024), B), dim3(256), 0, s, x, L, coef, y);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

// ---------------------------------------------------------------------------------
// Utterance length policy as one batched device op (data/test_set.py:139-146 `pad`,
// :201-227 `adjustDuration`, :229-248 `adjustDuration_random_start`): all three are
//     out[b][i] = x_b[(start_b + i) mod n_b],   i < duration
// (a short clip is repeated whole plus a residue, a long one is cropped from start_b; start_b = 0
// for the first-N policies).  x is the ragged batch packed back to back, offs[b] .. offs[b+1] its
// sample range.
// ---------------------------------------------------------------------------------
__global__ void tile_crop_kernel(const float* __restrict__ x, const long long* __restrict__ offs,
                                 const long long* __restrict__ starts, int duration, float* __restrict__ out) {
  const int b = blockIdx.y;
  const long long o = offs[b], n = offs[b + 1] - o;
  long long p = starts ? starts[b] : 0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < duration; i += gridDim.x * blockDim.x)
    out[(long)b * duration + i] = x[o + (p + i) % n];
}
const char* launch_tile_crop(const float* x, const long long* offs, const long long* starts, int B, int duration,
                             float* out, hipStream_t s) {
  if (B <= 0 || duration <= 0) return "tile_crop: empty batch";
  hipLaunchKernelGGL(tile_crop_kernel, dim3(min((duration + 255) / 256, 256), B), dim3(256), 0, s, x, offs, starts,
                     duration, out);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

// ---------------------------------------------------------------------------------
// Polyphase resampling to 16 kHz (afx/resample.py; the function is stated in include/afx.h):
//     y[n] = sum_{j<T} taps[p][j] * v[i0 - j],   i0 = floor(n*M/L),  p = n*M mod L
// fp32 taps, one fmaf chain per output in ascending j.  ONE tile body, polyphase_tiles, computes it for the three kernels
// that resample: resample_kernel (whole clips, or rows of a stream hop by hop), ingest_kernel (encoded packets of any
// length) and jitter_release_kernel (a jitter buffer's reorder ring).  A kernel decodes and validates its own row, then
// hands the body the row's n_out outputs, a SOURCE (sample k of the row, k >= -(T-1) counted from the row's first new
// sample: before it come zeros, the slot's T-1 carried samples, or the ring itself) and a SINK (where output n of the row
// goes: linear, or a position of the slot's pending ring).  A row that continues a stream with N inputs received and
// n_done = ceil(N*L/M) outputs made passes p0 = n_done*M mod L and d0 = floor(n_done*M/L) - N >= 0 (p0 = d0 = 0: the
// stream's start, or a whole number of filter periods into it); output n of the row is output n_done + n of the stream:
//     y = sum_{j<T} taps[p][j] * v[i - j],   i = d0 + floor((n*M + p0)/L),  p = (n*M + p0) mod L
// Every output gets the same T inputs and taps in the same order whichever kernel makes it and however the stream was
// cut, so a stream resampled hop by hop, packet by packet or out of a jitter buffer is bit-identical to the whole signal
// resampled at once; with one body that holds by construction.
// Tiling: a workgroup owns `R` consecutive sub-tiles of 256 outputs of one row (one output per lane); per sub-tile it
// stages its input span v[i(n0) - (T-1) .. i(n0 + 255)] in LDS.  The (L, T) tap table is staged in LDS too (row stride Tp,
// odd, so lanes on different phases hit different banks) when it fits, else read from global memory.  Memory-bound: a
// 48 kHz input is read once, the 16 kHz output written once.
// ---------------------------------------------------------------------------------
constexpr int RS_TILE = 256;          // outputs per sub-tile (one per lane)
constexpr int RS_TAPS_LDS = 12288;    // largest L * Tp staged in LDS (48 KB)
constexpr int RS_SPAN_MAX = 4096;     // largest staged input span (16 KB): (255 M + L - 1) / L + T for M / L <= 12

struct PolyFilter {
  const float* taps;             // (L, T); nullptr = identity (ingest / jitter release)
  int L, M, T, Tp, R;            // Tp, R: set by poly_grid
};

// Idx: the type of a row's sample and output indices (long long where a row can pass 2^31, as the offline offsets can)
template <bool LDS_TAPS, class Idx, class Src, class Sink>
__device__ __forceinline__ void polyphase_tiles(const PolyFilter& f, Idx n_out, int p0r, Idx d0, Src src, Sink sink) {
  extern __shared__ __attribute__((aligned(16))) float rs_lds[];
  const int T = f.T;
  const float* tp = f.taps;
  int ts = T;
  float* xs = rs_lds;
  if (LDS_TAPS) {
    for (int k = threadIdx.x; k < f.L * f.Tp; k += blockDim.x) {
      const int p = k / f.Tp, j = k - p * f.Tp;
      rs_lds[k] = j < T ? f.taps[p * T + j] : 0.f;
    }
    tp = rs_lds;
    ts = f.Tp;
    xs = rs_lds + f.L * f.Tp;
  }
  for (int r = 0; r < f.R; ++r) {
    const Idx n0 = ((Idx)blockIdx.x * f.R + r) * RS_TILE;
    if (n0 >= n_out) break;
    const int cnt = (int)min((Idx)RS_TILE, n_out - n0);
    const long long q0 = (long long)n0 * f.M + p0r, b0 = q0 / f.L;
    const int p0 = (int)(q0 - b0 * f.L);
    const Idx base = d0 + (Idx)b0;  // the row position of output n0's newest input
    // inputs base - (T-1) .. i(n0 + cnt - 1), which is inside the row for every output the host counted
    const int span = (int)(((long long)(cnt - 1) * f.M + p0) / f.L) + T;
    __syncthreads();  // the previous sub-tile is done with xs
    for (int s = threadIdx.x; s < span; s += blockDim.x) xs[s] = src(base - (T - 1) + s);
    __syncthreads();
    const int t = threadIdx.x;
    if (t < cnt) {
      const unsigned q = (unsigned)t * (unsigned)f.M + (unsigned)p0;
      const int di = (int)(q / (unsigned)f.L), p = (int)(q - (unsigned)di * (unsigned)f.L);
      const float* w = tp + (long)p * ts;
      const float* xv = xs + di + T - 1;
      float acc = 0.f;
      for (int j = 0; j < T; ++j) acc = __builtin_fmaf(w[j], xv[-j], acc);
      sink(n0 + t, acc);
    }
  }
}

// the carried samples of a row's slot after the row: the last H = T-1 of h ++ the row's n_in samples.  One workgroup per
// row (the slots of a launch are distinct): every lane reads its new value before any lane writes, so the in-place shift
// of a row shorter than H does not race.
template <class Src>
__device__ __forceinline__ void hist_shift(float* h, int H, int n_in, Src src) {
  const int k = threadIdx.x;
  float v = 0.f;
  if (k < H) v = (long long)k + n_in < H ? h[k + n_in] : src(k + n_in - H);
  __syncthreads();
  if (k < H) h[k] = v;
}

// the launch shape of polyphase_tiles for rows of up to max_out > 0 outputs: f.Tp, f.R and the grid's x, LDS bytes and
// tap placement; false for a ratio whose input span does not fit
struct PolyGrid { bool lds_taps; size_t lds; long long gx; };
static bool poly_grid(PolyFilter& f, bool ident, long long max_out, PolyGrid& g) {
  const long long span = (255LL * f.M + f.L - 1) / f.L + f.T;
  if (span > RS_SPAN_MAX) return false;
  f.Tp = f.T | 1;
  g.lds_taps = !ident && (long long)f.L * f.Tp <= RS_TAPS_LDS;
  f.R = g.lds_taps ? max(1, min(8, f.L * f.Tp / 1024)) : 1;  // amortise the tap staging of many-phase ratios
  g.gx = (max_out + (long long)RS_TILE * f.R - 1) / ((long long)RS_TILE * f.R);
  g.lds = ident ? 0 : sizeof(float) * (size_t)((g.lds_taps ? f.L * f.Tp : 0) + span);
  return true;
}

// sample k of a dense fp32 row, with the slot's carried samples (HIST: the H before it, oldest first) or zeros before it
template <bool HIST>
struct DenseSource {
  const float* x;
  const float* hrow;
  int H;
  __device__ __forceinline__ float operator()(long long k) const { return k >= 0 ? x[k] : (HIST ? hrow[H + k] : 0.f); }
};
struct LinearSink {
  float* out;
  __device__ __forceinline__ void operator()(long long n, float v) const { out[n] = v; }
};
// output n of a row at position (wpos + n) mod len of the slot's pending ring (n < len)
struct RingSink {
  float* out;
  int wpos, len;
  __device__ __forceinline__ void operator()(int n, float v) const {
    const int w = wpos + n;
    out[w < len ? w : w - len] = v;
  }
};

struct ResampleArgs {
  const float* x;                // offline: clips packed back to back; streaming: (A, n_in) rows
  const long long* in_offs;      // offline: input offsets (B + 1)
  const long long* out_offs;     // offline: output offsets (B + 1)
  const float* hist;             // streaming: (S, T - 1) carried samples, oldest first
  const int* slot;               // streaming: row -> hist row
  PolyFilter f;
  int n_in;
  float* out;
};

// offline (zeros before a clip) and streamed (hist[slot[row]] before a row): p0 = d0 = 0
template <bool STREAM, bool LDS_TAPS>
__global__ __launch_bounds__(256) void resample_kernel(ResampleArgs a) {
  const int row = blockIdx.y, H = a.f.T - 1;
  long long in_base, out_base, n_out;
  if (STREAM) {
    n_out = (long long)a.n_in * a.f.L / a.f.M;
    in_base = (long long)row * a.n_in;
    out_base = (long long)row * n_out;
  } else {
    in_base = a.in_offs[row];
    out_base = a.out_offs[row];
    n_out = a.out_offs[row + 1] - out_base;
  }
  const DenseSource<STREAM> src{a.x + in_base, STREAM ? a.hist + (long long)a.slot[row] * H : nullptr, H};
  polyphase_tiles<LDS_TAPS>(a.f, n_out, 0, 0LL, src, LinearSink{a.out + out_base});
}

__global__ __launch_bounds__(256) void resample_hist_kernel(const float* __restrict__ x, int n_in, const int* __restrict__ slot,
                                                            int H, float* hist) {
  const int row = blockIdx.x;
  hist_shift(hist + (long long)slot[row] * H, H, n_in, DenseSource<false>{x + (long long)row * n_in, nullptr, 0});
}

static const char* launch_resample_any(bool stream, ResampleArgs a, int rows, long long max_out, hipStream_t s) {
  if (a.f.L <= 0 || a.f.M <= 0 || a.f.T <= 0 || !a.f.taps || !a.x || !a.out) return "resample: bad arguments";
  if (rows <= 0 || rows > 65535) return "resample: 1 to 65535 rows";
  if (max_out <= 0) return nullptr;
  PolyGrid g;
  if (!poly_grid(a.f, false, max_out, g)) return "resample: input / output ratio above 12";
  if (g.gx > 0x7fffffffLL) return "resample: too many outputs per row";
  const dim3 grid((unsigned)g.gx, rows);
  if (stream && g.lds_taps) hipLaunchKernelGGL((resample_kernel<true, true>), grid, dim3(256), g.lds, s, a);
  else if (stream) hipLaunchKernelGGL((resample_kernel<true, false>), grid, dim3(256), g.lds, s, a);
  else if (g.lds_taps) hipLaunchKernelGGL((resample_kernel<false, true>), grid, dim3(256), g.lds, s, a);
  else hipLaunchKernelGGL((resample_kernel<false, false>), grid, dim3(256), g.lds, s, a);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

const char* launch_resample(const float* x, const long long* in_offs, const long long* out_offs, int B, long long max_out,
                            const float* taps, int L, int M, int T, float* out, hipStream_t s) {
  if (!in_offs || !out_offs) return "resample: null offsets";
  ResampleArgs a{};
  a.x = x; a.in_offs = in_offs; a.out_offs = out_offs; a.f = PolyFilter{taps, L, M, T, 0, 0}; a.out = out;
  return launch_resample_any(false, a, B, max_out, s);
}

const char* launch_resample_stream(const float* x, int A, int n_in, float* hist, const int* slot, const float* taps, int L,
                                   int M, int T, float* out, hipStream_t s) {
  if (!hist || !slot) return "resample_stream: null history or slot table";
  if (n_in <= 0 || M <= 0 || ((long long)n_in * L) % M != 0) return "resample_stream: n_in * L must be a multiple of M";
  if (T - 1 > 256) return "resample_stream: more than 256 carried samples";
  ResampleArgs a{};
  a.x = x; a.hist = hist; a.slot = slot; a.f = PolyFilter{taps, L, M, T, 0, 0}; a.n_in = n_in; a.out = out;
  const char* m = launch_resample_any(true, a, A, (long long)n_in * L / M, s);
  if (m || T == 1) return m;
  hipLaunchKernelGGL(resample_hist_kernel, dim3(A), dim3(256), 0, s, x, n_in, slot, T - 1, hist);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

// ---------------------------------------------------------------------------------
// Packet ingest (afx/ingest.py; the function is stated in include/afx.h afx_k_ingest / afx_k_ingest_pop): each row is the
// next n_in encoded samples of one slot's stream, of any length, starting at any filter phase.  The row's header carries
// n_out, p0 and d0 as the host reduced them from the stream's absolute counters; ingest_kernel is polyphase_tiles (above)
// with the source = the packet decoded (exact in fp32), hist[slot] at negative positions, and the sink = the slot's
// pending ring from wpos on.  A second kernel then makes hist[slot] the last T-1 decoded samples of hist ++ packet.
// taps == nullptr: the identity (16 kHz input), sample k decoded straight into the ring.
// ---------------------------------------------------------------------------------
constexpr int ING_HDR = 8;  // ints per row: slot, byte offset of the first sample, n_in, n_out, p0, d0, wpos, 0

struct IngestArgs {
  const unsigned char* stage;    // encoded payloads (each row's first sample at its header's byte offset)
  long long stage_bytes;
  const int* hdr;                // (rows, ING_HDR)
  PolyFilter f;
  float* hist;                   // (S, T - 1)
  float* ring;                   // (S, ring_len)
  int enc, S, ring_len;
};

// sample k of an encoded payload as fp32 (exact: 16-bit linear value / 32768; ITU-T G.711 expansion)
__device__ __forceinline__ float ingest_sample(const unsigned char* p, int k, int enc) {
  if (enc == 0) return ((const float*)p)[k];
  int v;
  if (enc == 1) {
    v = ((const short*)p)[k];
  } else if (enc == 2) {
    const int u = ~(int)p[k] & 0xFF;
    v = ((((u & 15) << 3) + 132) << ((u >> 4) & 7)) - 132;
    if (u & 0x80) v = -v;
  } else {
    const int a = (int)p[k] ^ 0x55, e = (a >> 4) & 7, m = (a & 15) << 4;
    v = e ? (m + 264) << (e - 1) : m + 8;
    if (!(a & 0x80)) v = -v;
  }
  return (float)v * (1.0f / 32768.0f);
}

__device__ __forceinline__ int ingest_bytes_per_sample(int enc) { return enc == 0 ? 4 : enc == 1 ? 2 : 1; }

// the row's header, or false for a row that would leave its buffers (the host plans every field; nothing is written then)
__device__ __forceinline__ bool ingest_row(const IngestArgs& a, int row, int& slot, const unsigned char*& pay, int& n_in,
                                           int& n_out, int& p0, int& d0, int& wpos) {
  const int* h = a.hdr + (long long)row * ING_HDR;
  slot = h[0]; n_in = h[2]; n_out = h[3]; p0 = h[4]; d0 = h[5]; wpos = h[6];
  const long long off = h[1];
  pay = a.stage + off;
  const int bps = ingest_bytes_per_sample(a.enc);
  return slot >= 0 && slot < a.S && n_in >= 0 && n_out >= 0 && n_out <= a.ring_len && wpos >= 0 && wpos < a.ring_len &&
         p0 >= 0 && p0 < a.f.L && d0 >= 0 && off >= 0 && (off & (bps - 1)) == 0 && off + (long long)n_in * bps <= a.stage_bytes;
}

// sample k of a packet decoded (zeros past its end: never reached by an output the host counted), the slot's carried
// samples before it
struct PacketSource {
  const unsigned char* pay;
  int enc, n_in;
  const float* hrow;
  int H;
  __device__ __forceinline__ float operator()(int k) const {
    return k >= 0 ? (k < n_in ? ingest_sample(pay, k, enc) : 0.f) : hrow[H + k];
  }
};

// one row of an ingest launch; hs: the row stride of hist (T - 1, or the widest T - 1 of a scorer of several formats: a slot
// then uses the first T - 1 columns of its row)
template <bool IDENT, bool LDS_TAPS>
__device__ __forceinline__ void ingest_tiles(const IngestArgs& a, int row, int hs) {
  int slot, n_in, n_out, p0, d0, wpos;
  const unsigned char* pay;
  if (!ingest_row(a, row, slot, pay, n_in, n_out, p0, d0, wpos)) return;
  float* out = a.ring + (long long)slot * a.ring_len;
  if (IDENT) {
    for (int r = 0; r < a.f.R; ++r) {
      const int k = (blockIdx.x * a.f.R + r) * RS_TILE + threadIdx.x;
      if (k >= n_out || k >= n_in) break;
      const int w = wpos + k;
      out[w < a.ring_len ? w : w - a.ring_len] = ingest_sample(pay, k, a.enc);
    }
    return;
  }
  if ((long long)blockIdx.x * a.f.R * RS_TILE >= n_out) return;  // (a short row of a ragged launch: no taps staged for it)
  const int H = a.f.T - 1;
  polyphase_tiles<LDS_TAPS>(a.f, n_out, p0, d0, PacketSource{pay, a.enc, n_in, a.hist + (long long)slot * hs, H},
                            RingSink{out, wpos, a.ring_len});
}

__device__ __forceinline__ void ingest_hist_row(const IngestArgs& a, int row, int hs) {
  int slot, n_in, n_out, p0, d0, wpos;
  const unsigned char* pay;
  if (!ingest_row(a, row, slot, pay, n_in, n_out, p0, d0, wpos)) return;
  hist_shift(a.hist + (long long)slot * hs, a.f.T - 1, n_in, PacketSource{pay, a.enc, n_in, nullptr, 0});
}

template <bool IDENT, bool LDS_TAPS>
__global__ __launch_bounds__(256) void ingest_kernel(IngestArgs a) {
  ingest_tiles<IDENT, LDS_TAPS>(a, blockIdx.y, a.f.T - 1);
}

__global__ __launch_bounds__(256) void ingest_hist_kernel(IngestArgs a) { ingest_hist_row(a, blockIdx.x, a.f.T - 1); }

const char* launch_ingest(const void* stage, long long stage_bytes, const int* hdr, int rows, int max_out, int enc,
                          const float* taps, int L, int M, int T, float* hist, float* ring, int S, int ring_len,
                          hipStream_t s) {
  if (!stage || !hdr || !ring || stage_bytes <= 0) return "ingest: null staging buffer, header table or ring";
  if (enc < 0 || enc > 3) return "ingest: encoding 0 (pcm_f32le), 1 (pcm_s16le), 2 (mulaw) or 3 (alaw)";
  if (rows <= 0 || rows > 65535) return "ingest: 1 to 65535 rows";
  if (S <= 0 || ring_len <= 0 || max_out < 0 || max_out > ring_len) return "ingest: a row's outputs must fit its slot's ring";
  if (L <= 0 || M <= 0 || T <= 0) return "ingest: bad filter shape";
  const bool ident = taps == nullptr;
  if (ident && (L != 1 || M != 1 || T != 1)) return "ingest: no taps is the identity (L = M = T = 1)";
  if (!ident && T > 1 && !hist) return "ingest: null history";
  if (T - 1 > 256) return "ingest: more than 256 carried samples";
  IngestArgs a{};
  a.stage = (const unsigned char*)stage; a.stage_bytes = stage_bytes; a.hdr = hdr; a.hist = hist; a.ring = ring;
  a.f = PolyFilter{taps, L, M, T, 0, 0}; a.enc = enc; a.S = S; a.ring_len = ring_len;
  if (max_out > 0) {
    PolyGrid g;
    if (!poly_grid(a.f, ident, max_out, g)) return "ingest: input / output ratio above 12";
    const dim3 grid((unsigned)g.gx, rows);
    if (ident) hipLaunchKernelGGL((ingest_kernel<true, false>), grid, dim3(256), g.lds, s, a);
    else if (g.lds_taps) hipLaunchKernelGGL((ingest_kernel<false, true>), grid, dim3(256), g.lds, s, a);
    else hipLaunchKernelGGL((ingest_kernel<false, false>), grid, dim3(256), g.lds, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hipGetErrorString(e);
  }
  if (T == 1) return nullptr;
  hipLaunchKernelGGL(ingest_hist_kernel, dim3(rows), dim3(256), 0, s, a);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

// ---------------------------------------------------------------------------------
// Packet ingest over rows of different formats (afx/ingest.py MixedPacketScorer; include/afx.h afx_k_ingest_mixed): the
// format (encoding, taps, L, M, T) is a per-row value, the eighth int of the row's header, instead of a launch-wide one.  The
// table of a scorer's formats (at most ING_MAX_FORMATS) travels by value in the argument struct; a workgroup reads its row's
// entry, makes the row's IngestArgs of it and runs ingest_tiles / ingest_hist_row above: the same validation, decoder, tile
// body and history shift, so every output comes from the fmaf chain a one-format launch gives it.  The branch on the tap
// placement is uniform per workgroup.  hist is (S, Hs), Hs >= every format's T - 1.
// ---------------------------------------------------------------------------------
constexpr int ING_MAX_FORMATS = 16;

struct IngestFormat {
  PolyFilter f;                  // Tp, R from poly_grid
  int enc, lds_taps;             // taps == nullptr: the identity
};

struct IngestMixedArgs {
  const unsigned char* stage;
  long long stage_bytes;
  const int* hdr;                // (rows, ING_HDR), the eighth int = the row's format
  float* hist;                   // (S, Hs)
  float* ring;                   // (S, ring_len)
  int S, ring_len, Hs, nf;
  IngestFormat fmt[ING_MAX_FORMATS];
};

// the launch's arguments as one row's format sees them; false for a format index outside the table
__device__ __forceinline__ bool ingest_mixed_row(const IngestMixedArgs& m, int row, IngestArgs& a, int& lds_taps) {
  const int fi = __builtin_amdgcn_readfirstlane(m.hdr[(long long)row * ING_HDR + 7]);
  if (fi < 0 || fi >= m.nf) return false;
  a.stage = m.stage; a.stage_bytes = m.stage_bytes; a.hdr = m.hdr; a.f = m.fmt[fi].f; a.hist = m.hist; a.ring = m.ring;
  a.enc = m.fmt[fi].enc; a.S = m.S; a.ring_len = m.ring_len;
  lds_taps = m.fmt[fi].lds_taps;
  return true;
}

__global__ __launch_bounds__(256) void ingest_mixed_kernel(IngestMixedArgs m) {
  IngestArgs a;
  int lds_taps;
  if (!ingest_mixed_row(m, blockIdx.y, a, lds_taps)) return;
  if (!a.f.taps) ingest_tiles<true, false>(a, blockIdx.y, m.Hs);
  else if (lds_taps) ingest_tiles<false, true>(a, blockIdx.y, m.Hs);
  else ingest_tiles<false, false>(a, blockIdx.y, m.Hs);
}

__global__ __launch_bounds__(256) void ingest_mixed_hist_kernel(IngestMixedArgs m) {
  IngestArgs a;
  int lds_taps;
  if (!ingest_mixed_row(m, blockIdx.x, a, lds_taps) || a.f.T == 1) return;
  ingest_hist_row(a, blockIdx.x, m.Hs);
}

const char* launch_ingest_mixed(const void* stage, long long stage_bytes, const int* hdr, int rows, const IngestFormatDesc* formats,
                                int n_formats, const int* max_out, float* hist, int Hs, float* ring, int S, int ring_len,
                                hipStream_t s) {
  if (n_formats < 1 || n_formats > ING_MAX_FORMATS) return "ingest_mixed: 1 to 16 formats";
  if (!formats || !max_out) return "ingest_mixed: null format table or output counts";
  IngestMixedArgs m{};
  PolyGrid g[ING_MAX_FORMATS];
  bool carried = false;
  for (int i = 0; i < n_formats; ++i) {
    const IngestFormatDesc& d = formats[i];
    if (d.encoding < 0 || d.encoding > 3) return "ingest_mixed: encoding 0 (pcm_f32le), 1 (pcm_s16le), 2 (mulaw) or 3 (alaw)";
    if (d.L <= 0 || d.M <= 0 || d.T <= 0) return "ingest_mixed: bad filter shape";
    const bool ident = d.taps == nullptr;
    if (ident && (d.L != 1 || d.M != 1 || d.T != 1)) return "ingest_mixed: bad filter shape (no taps is the identity, L = M = T = 1)";
    if (d.T - 1 > 256) return "ingest_mixed: more than 256 carried samples";
    m.fmt[i].f = PolyFilter{d.taps, d.L, d.M, d.T, 0, 0};
    m.fmt[i].enc = d.encoding;
    if (!poly_grid(m.fmt[i].f, ident, max_out[i] > 0 ? max_out[i] : 0, g[i])) return "ingest_mixed: input / output ratio above 12";
    m.fmt[i].lds_taps = g[i].lds_taps;
    carried = carried || d.T > 1;
  }
  if (!stage || !hdr || !ring || stage_bytes <= 0) return "ingest_mixed: null staging buffer, header table or ring";
  if (rows <= 0 || rows > 65535) return "ingest_mixed: 1 to 65535 rows";
  if (S <= 0 || ring_len <= 0) return "ingest_mixed: a row's outputs must fit its slot's ring";
  long long gx = 0;
  size_t lds = 0;
  for (int i = 0; i < n_formats; ++i) {
    if (max_out[i] < 0 || max_out[i] > ring_len) return "ingest_mixed: a row's outputs must fit its slot's ring";
    if (formats[i].T - 1 > Hs) return "ingest_mixed: the history rows are narrower than a format's T - 1";
    if (max_out[i] > 0) {
      gx = g[i].gx > gx ? g[i].gx : gx;
      lds = g[i].lds > lds ? g[i].lds : lds;
    }
  }
  if (carried && !hist) return "ingest_mixed: null history";
  m.stage = (const unsigned char*)stage; m.stage_bytes = stage_bytes; m.hdr = hdr; m.hist = hist; m.ring = ring;
  m.S = S; m.ring_len = ring_len; m.Hs = Hs; m.nf = n_formats;
  if (gx > 0) {
    hipLaunchKernelGGL(ingest_mixed_kernel, dim3((unsigned)gx, rows), dim3(256), lds, s, m);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hipGetErrorString(e);
  }
  if (!carried) return nullptr;
  hipLaunchKernelGGL(ingest_mixed_hist_kernel, dim3(rows), dim3(256), 0, s, m);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

// the first `hop` pending samples of the named slots: out[i][k] = ring[slot_i][(head_i + k) mod ring_len], table (A, 2)
// int32 = (slot_i, head_i).  The ring is only read: head and fill are the host's.
__global__ __launch_bounds__(256) void ingest_pop_kernel(const float* __restrict__ ring, int S, int ring_len,
                                                         const int* __restrict__ table, int hop, float* __restrict__ out) {
  const int row = blockIdx.y, slot = table[2 * row], head = table[2 * row + 1];
  const bool ok = slot >= 0 && slot < S && head >= 0 && head < ring_len;
  const float* src = ring + (long long)(ok ? slot : 0) * ring_len;
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < hop; k += gridDim.x * blockDim.x) {
    const int w = head + k;
    out[(long long)row * hop + k] = ok ? src[w < ring_len ? w : w - ring_len] : 0.f;
  }
}

const char* launch_ingest_pop(const float* ring, int S, int ring_len, const int* table, int A, int hop, float* out,
                              hipStream_t s) {
  if (!ring || !table || !out) return "ingest_pop: null argument";
  if (S <= 0 || A <= 0 || A > 65535) return "ingest_pop: 1 to 65535 rows";
  if (hop <= 0 || hop > ring_len) return "ingest_pop: a hop must fit the ring";
  hipLaunchKernelGGL(ingest_pop_kernel, dim3(min((hop + 255) / 256, 64), A), dim3(256), 0, s, ring, S, ring_len, table, hop, out);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

// ---------------------------------------------------------------------------------
// Payload expand (afx/codecs.py; the function is stated in include/afx.h afx_k_payload_expand): the verb that runs before
// ingest / place.  The kernels above read a payload by random access (ingest_sample); a payload they cannot index that way
// -- DVI4 is a recurrence within its block, network-order PCM needs its bytes put together -- is first written as fp32
// samples into another zone of the same staging buffer, and read from there as encoding 0.  One workgroup of ONE wave per
// (column of the grid, row); a row's codec is uniform over its workgroups, so every branch below is.
//   PCM codecs: a grid-stride map over the row's samples.
//   DVI4: the wave of grid column 0 walks the block 64 codes a step and carries the concrete (pred, index) from step to step.
//   Within a step both recurrences are prefix scans over clamp-add maps x -> min(max(x + a, lo), hi), which are closed under
//   composition (clamp_then): an exclusive scan of the index maps gives each lane its index, the lane looks up its step size
//   (table in LDS) and forms +-d, an inclusive scan of the predictor maps gives its pred.  Integer VALU and __shfl_up only;
//   over 64 codes |a| <= 64 * 61438 and the sentinels of the identity stay inside +-2^29, so nothing overflows int32.
// ---------------------------------------------------------------------------------
constexpr int EXP_HDR = 4;  // ints per row: source byte offset, source bytes, destination byte offset, codec number
constexpr int EXP_DVI4 = 0, EXP_S16BE = 1, EXP_S24BE = 2, EXP_U8 = 3;
constexpr int EXP_INF = 1 << 28;  // the bounds of a map that does not clamp

__constant__ int DVI4_STEP[89] = {
    7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45, 50, 55, 60, 66, 73, 80, 88, 97, 107, 118, 130, 143,
    157, 173, 190, 209, 230, 253, 279, 307, 337, 371, 408, 449, 494, 544, 598, 658, 724, 796, 876, 963, 1060, 1166, 1282, 1411,
    1552, 1707, 1878, 2066, 2272, 2499, 2749, 3024, 3327, 3660, 4026, 4428, 4871, 5358, 5894, 6484, 7132, 7845, 8630, 9493, 10442,
    11487, 12635, 13899, 15289, 16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767};

struct ClampAdd { int a, lo, hi; };  // x -> min(max(x + a, lo), hi), lo <= hi

__device__ __forceinline__ int clamp_int(int x, int lo, int hi) { return min(max(x, lo), hi); }
__device__ __forceinline__ int clamp_apply(const ClampAdd& m, int x) { return clamp_int(x + m.a, m.lo, m.hi); }
// g after f
__device__ __forceinline__ ClampAdd clamp_then(const ClampAdd& f, const ClampAdd& g) {
  return ClampAdd{f.a + g.a, clamp_int(f.lo + g.a, g.lo, g.hi), clamp_int(f.hi + g.a, g.lo, g.hi)};
}
// lane i: the composition of the maps of lanes 0..i, in lane order (the block is one wave of 64)
__device__ __forceinline__ ClampAdd clamp_scan(ClampAdd m, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const ClampAdd f{__shfl_up(m.a, d, 64), __shfl_up(m.lo, d, 64), __shfl_up(m.hi, d, 64)};
    if (lane >= d) m = clamp_then(f, m);
  }
  return m;
}

// one DVI4 block (RFC 3551 4.5.1) of n = 2 (bytes - 4) codes, header validated by the caller -> out[0..n)
__device__ __forceinline__ void expand_dvi4(const unsigned char* src, int n, float* out, const int* steps) {
  const int lane = threadIdx.x;
  int pred = (short)((src[0] << 8) | src[1]), index = src[2];
  for (int base = 0; base < n; base += 64) {
    const int k = base + lane;
    const bool active = k < n;
    int c = 0;
    if (active) {
      const int b = src[4 + (k >> 1)];
      c = (k & 1) ? (b & 15) : (b >> 4);  // the high nibble first
    }
    const ClampAdd none{0, -EXP_INF, EXP_INF};
    const ClampAdd im = clamp_scan(active ? ClampAdd{(c & 7) < 4 ? -1 : ((c & 7) - 3) * 2, 0, 88} : none, lane);
    const int after = clamp_apply(im, index);  // the index after this lane's code
    int mine = __shfl_up(after, 1, 64);        // the index this lane's code is decoded with
    if (lane == 0) mine = index;
    const int st = steps[mine];
    const int d = (st >> 3) + ((c & 4) ? st : 0) + ((c & 2) ? st >> 1 : 0) + ((c & 1) ? st >> 2 : 0);
    const ClampAdd pm = clamp_scan(active ? ClampAdd{(c & 8) ? -d : d, -32768, 32767} : none, lane);
    const int p = clamp_apply(pm, pred);
    if (active) out[k] = (float)p * (1.0f / 32768.0f);
    index = __shfl(after, 63, 64);  // (lanes past the block's end are the identity: lane 63 holds the state after the last code)
    pred = __shfl(p, 63, 64);
  }
}

// a row that has a bad codec, splits a sample, is a malformed DVI4 block or leaves stage is skipped whole: nothing is written
__global__ __launch_bounds__(64) void payload_expand_kernel(unsigned char* stage, long long stage_bytes, const int* __restrict__ hdr) {
  __shared__ int steps[89];
  const int* h = hdr + (long long)blockIdx.y * EXP_HDR;
  const long long src_off = h[0], nbytes = h[1], dst_off = h[2];
  const int codec = __builtin_amdgcn_readfirstlane(h[3]);
  if (codec < EXP_DVI4 || codec > EXP_U8 || src_off < 0 || nbytes < 0 || src_off + nbytes > stage_bytes) return;
  const unsigned char* src = stage + src_off;
  long long n;
  if (codec == EXP_DVI4) {
    if (nbytes < 4 || src[2] > 88) return;
    n = 2 * (nbytes - 4);
  } else {
    const int unit = codec == EXP_S16BE ? 2 : codec == EXP_S24BE ? 3 : 1;
    if (nbytes % unit) return;
    n = nbytes / unit;
  }
  if (dst_off < 0 || (dst_off & 3) || dst_off + 4 * n > stage_bytes) return;
  float* out = (float*)(stage + dst_off);
  if (codec == EXP_DVI4) {
    if (blockIdx.x) return;
    for (int i = threadIdx.x; i < 89; i += 64) steps[i] = DVI4_STEP[i];
    __syncthreads();
    expand_dvi4(src, (int)n, out, steps);
    return;
  }
  for (long long k = (long long)blockIdx.x * 64 + threadIdx.x; k < n; k += (long long)gridDim.x * 64) {
    if (codec == EXP_S16BE) {
      out[k] = (float)(short)((src[2 * k] << 8) | src[2 * k + 1]) * (1.0f / 32768.0f);
    } else if (codec == EXP_S24BE) {
      const int v = ((int)(signed char)src[3 * k] << 16) | (src[3 * k + 1] << 8) | src[3 * k + 2];
      out[k] = (float)v * (1.0f / 8388608.0f);
    } else {
      out[k] = (float)((int)src[k] - 128) * (1.0f / 128.0f);
    }
  }
}

const char* launch_payload_expand(void* stage, long long stage_bytes, const int* hdr, int rows, int max_n, hipStream_t s) {
  if (!stage || !hdr || stage_bytes <= 0) return "afx_k_payload_expand: null staging buffer or header table";
  if (rows <= 0 || rows > 65535) return "afx_k_payload_expand: 1 to 65535 rows";
  if (max_n < 0 || 4LL * max_n > stage_bytes) return "afx_k_payload_expand: a row's samples must fit the staging buffer";
  if (max_n == 0) return nullptr;  // no samples to write
  hipLaunchKernelGGL(payload_expand_kernel, dim3(min((max_n + 255) / 256, 64), rows), dim3(64), 0, s, (unsigned char*)stage,
                     stage_bytes, hdr);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

// ---------------------------------------------------------------------------------
// Jitter buffer (afx/jitter.py; the functions are stated in include/afx.h afx_k_jitter_place / _conceal / _release and their
// _mixed / _rates forms): one DECODED reorder ring per slot, jring (S, Js) fp32.  A slot has a RATE: its filter (taps, L, M, T),
// its ring length J <= Js, its repeat period P, fade length F and fade table.  Input-rate sample i of the slot's played-out
// stream E sits at column i mod J of its row; the slot uses the columns [0, J) only and never touches one at or beyond J.
// The host keeps every index (playout point `next`, received intervals, gaps) and plans rounds so that, with
// lookback = max(T - 1, P + F) and W = J - lookback, every launch of a round that has released E up to `cur` touches only
// indices in [cur - lookback, cur + W): a window of J consecutive indices, so no two of them share a column.  That is the
// sizing invariant: what place writes at i >= cur destroys only i - J < cur - lookback, which neither the filter (T - 1
// samples back) nor a fading gap (source [a - P, a), read until a + F) will read again.
// Four verbs, one kernel and one row body each:
//   place:   decodes sub-ranges of packets into their columns (the rows of one launch are disjoint: the host splits a packet
//            at the playout point and at what was received before; first arrival wins).
//   conceal: writes a released gap's samples INTO the ring (zeros, or the faded repetition of the P samples before the
//            gap), so that a later gap, and the filter, read them as they read received samples.  Gaps of one slot are
//            ordered by the host: one launch per rank of gap within the slot.
//   noise:   writes the comfort-noise part of a released gap INTO the ring (RFC 3389 silence, afx_k_jitter_noise): a hash
//            of the 64-bit stream index and the seed times the level's amplitude.  No source, so no ranks: one launch per
//            round, before the conceal ranks (a loss gap whose source holds this round's noise then reads it).
//   release: polyphase_tiles (above) with the source = ring[(a0 + k) mod J], k >= -(T-1), and the sink = the slot's pending
//            16 kHz ring: outputs n_done .. of the stream, each with the bits afx_k_resample gives it over all of E.
// The rates of a launch (at most JIT_MAX_RATES) travel by value in the argument struct; a row names its rate by an index, the
// last int of its header, or, in a launch whose rows carry none (the one-rate entry points: a table of one entry, Js = J), is
// at rate 0.  A workgroup reads its row's entry (the index made wave-uniform, so the entry is scalar loads from the kernel
// arguments) and runs the row body with that rate's values; the branch on the tap placement is uniform per workgroup.
// ---------------------------------------------------------------------------------
constexpr int JIT_MAX_RATES = 16;
// ints per row.  place: slot, byte offset of the first sample, n, ring column of the first sample [, encoding [, rate index]];
// conceal: slot, ring column of the gap origin a, d_lo, d_hi [, rate index]; release: slot, ring column of a0, n_in, n_out,
// p0, d0, wpos, rate index (read only where the launch says its rows carry one)
constexpr int JIT_PLACE_HDR = 4, JIT_PLACE_MIXED_HDR = 5, JIT_PLACE_RATES_HDR = 6;
constexpr int JIT_CONCEAL_HDR = 4, JIT_CONCEAL_RATES_HDR = 5;
constexpr int JIT_RELEASE_HDR = 8;
// noise: slot, ring column of the first index, n, lo32(i0), hi32(i0), level [, rate index]
constexpr int JIT_NOISE_HDR = 6, JIT_NOISE_RATES_HDR = 7;

struct JitterRate {
  PolyFilter f;                  // Tp, R from poly_grid (release only)
  const float* fade;             // (max(F, 1),) fp32 (conceal only)
  int J, P, F, lds_taps;
  int max_out;                   // release: the largest n_out the launch was shaped for (a row beyond it writes nothing)
};

struct JitterRatesArgs {
  const unsigned char* stage;    // place
  long long stage_bytes;
  const int* hdr;                // (rows, hdr_ints)
  float* jring;                  // (S, Js)
  float* ring;                   // release: (S, ring_len) pending 16 kHz samples
  int S, Js, ring_len, nr, mode;
  int hdr_ints;                  // the row stride
  int enc;                       // place: the encoding of rows of JIT_PLACE_HDR ints (longer rows name their own, the fifth int)
  int rated;                     // the last int of a row is its rate index (else every row is at rate 0)
  unsigned seed;                 // noise
  const float* amp;              // noise: (128,) fp32, the amplitude of each level
  JitterRate r[JIT_MAX_RATES];
};

// the calling workgroup's row and its rate index (the caller checks its range)
__device__ __forceinline__ const int* jitter_row(const JitterRatesArgs& m, int& ri) {
  const int* h = m.hdr + (long long)blockIdx.y * m.hdr_ints;
  ri = m.rated ? __builtin_amdgcn_readfirstlane(h[m.hdr_ints - 1]) : 0;
  return h;
}

// one row of a place launch: h[0..3] = slot, byte offset, n, column; enc the row's encoding (validated by the caller); the
// slot's ring is the first J columns of a row of `stride` floats
__device__ __forceinline__ void jitter_place_row(const unsigned char* __restrict__ stage, long long stage_bytes, const int* h, int enc,
                                                 float* __restrict__ jring, int S, int J, int stride) {
  const int slot = h[0], n = h[2], col = h[3];
  const long long off = h[1];
  const int bps = ingest_bytes_per_sample(enc);
  if (!(slot >= 0 && slot < S && n >= 0 && n <= J && col >= 0 && col < J && off >= 0 && (off & (bps - 1)) == 0 &&
        off + (long long)n * bps <= stage_bytes))
    return;
  const unsigned char* pay = stage + off;
  float* row = jring + (long long)slot * stride;
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) {
    const int w = col + k;
    row[w < J ? w : w - J] = ingest_sample(pay, k, enc);
  }
}

// a row with a bad encoding or rate index is skipped whole
__global__ __launch_bounds__(256) void jitter_place_kernel(JitterRatesArgs m) {
  int ri;
  const int* h = jitter_row(m, ri);
  const int enc = m.hdr_ints > JIT_PLACE_HDR ? h[4] : m.enc;
  if (enc < 0 || enc > 3 || ri < 0 || ri >= m.nr) return;
  jitter_place_row(m.stage, m.stage_bytes, h, enc, m.jring, m.S, m.r[ri].J, m.Js);
}

// E[a + d] for d in [d_lo, d_hi): 0 (mode 0, or d >= F), else fade[d] * E[a - P + d mod P] (one fp32 multiply of two stored
// values).  The source columns [a - P, a) and the written ones [a + d_lo, a + d_hi) are disjoint for d_hi + P <= J.  One row of
// a conceal launch: h[0..3] = slot, column of a, d_lo, d_hi; the slot's ring is the first J columns of a row of `stride` floats.
__device__ __forceinline__ void jitter_conceal_row(float* __restrict__ jring, int S, int J, int stride, const int* h,
                                                   const float* __restrict__ fade, int P, int F, int mode) {
  const int slot = h[0], ac = h[1], lo = h[2], hi = h[3];
  if (!(slot >= 0 && slot < S && ac >= 0 && ac < J && lo >= 0 && hi >= lo && (long long)hi + P <= J)) return;
  float* row = jring + (long long)slot * stride;
  const int src0 = ac >= P ? ac - P : ac - P + J;
  for (int d = lo + blockIdx.x * blockDim.x + threadIdx.x; d < hi; d += gridDim.x * blockDim.x) {
    float v = 0.f;
    if (mode == 1 && d < F) {
      const int c = src0 + d % P;
      v = fade[d] * row[c < J ? c : c - J];
    }
    const int w = ac + d;  // < 2 J
    row[w < J ? w : w - J] = v;
  }
}

__global__ __launch_bounds__(256) void jitter_conceal_kernel(JitterRatesArgs m) {
  int ri;
  const int* h = jitter_row(m, ri);
  if (ri < 0 || ri >= m.nr) return;
  jitter_conceal_row(m.jring, m.S, m.r[ri].J, m.Js, h, m.r[ri].fade, m.r[ri].P, m.r[ri].F, m.mode);
}

// E[i] = amp * fp32(k(seed, i)): a 32-bit hash of the 64-bit index i (all integer arithmetic mod 2^32), its top 24 bits as
// a signed integer (exactly an fp32 number), one fp32 multiply
__device__ __forceinline__ float jitter_noise_value(unsigned long long i, unsigned seed, float amp) {
  unsigned x = (unsigned)i * 0x9E3779B9u + (unsigned)(i >> 32) * 0x85EBCA6Bu + seed;
  x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
  return amp * (float)((int)x >> 8);
}

// one row of a noise launch: h[0..5] = slot, column of index i0, n, lo32(i0), hi32(i0), level; the slot's ring is the first J
// columns of a row of `stride` floats
__device__ __forceinline__ void jitter_noise_row(float* __restrict__ jring, int S, int J, int stride, const int* h, unsigned seed,
                                                 const float* __restrict__ amp) {
  const int slot = h[0], col = h[1], n = h[2], level = h[5];
  if (!(slot >= 0 && slot < S && col >= 0 && col < J && n >= 0 && n <= J && level >= 0 && level <= 127 && h[4] >= 0)) return;
  const unsigned long long i0 = ((unsigned long long)(unsigned)h[4] << 32) | (unsigned)h[3];
  const float a = amp[level];
  float* row = jring + (long long)slot * stride;
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) {
    const int w = col + k;
    row[w < J ? w : w - J] = jitter_noise_value(i0 + (unsigned long long)k, seed, a);
  }
}

// a row with a bad rate index is skipped whole
__global__ __launch_bounds__(256) void jitter_noise_kernel(JitterRatesArgs m) {
  int ri;
  const int* h = jitter_row(m, ri);
  if (ri < 0 || ri >= m.nr) return;
  jitter_noise_row(m.jring, m.S, m.r[ri].J, m.Js, h, m.seed, m.amp);
}

// sample k of the released range that starts at ring column col0 (zeros past its end: never reached by an output the host
// counted); k >= -(T-1) >= -J and k < n_in <= J, so one wrap either way
struct RingSource {
  const float* src;
  int col0, J, n_in;
  __device__ __forceinline__ float operator()(int k) const {
    int c = col0 + k;
    c = c < 0 ? c + J : (c < J ? c : c - J);
    return k < n_in ? src[c] : 0.f;
  }
};

// one row of a release launch at a rate with filter f and ring length J: the identity copies, the others are polyphase_tiles
template <bool IDENT, bool LDS_TAPS>
__device__ __forceinline__ void jitter_release_row(const JitterRatesArgs& m, const PolyFilter& f, int J, const int* h) {
  const int slot = h[0], col0 = h[1], n_in = h[2], n_out = h[3], p0 = h[4], d0 = h[5], wpos = h[6];
  if (!(slot >= 0 && slot < m.S && col0 >= 0 && col0 < J && n_in >= 0 && n_in <= J && n_out >= 0 && n_out <= m.ring_len &&
        wpos >= 0 && wpos < m.ring_len && p0 >= 0 && p0 < f.L && d0 >= 0))
    return;
  const float* src = m.jring + (long long)slot * m.Js;
  float* out = m.ring + (long long)slot * m.ring_len;
  if (IDENT) {
    for (int r = 0; r < f.R; ++r) {
      const int k = (blockIdx.x * f.R + r) * RS_TILE + threadIdx.x;
      if (k >= n_out || k >= n_in) break;
      const int c = col0 + k, w = wpos + k;
      out[w < m.ring_len ? w : w - m.ring_len] = src[c < J ? c : c - J];
    }
    return;
  }
  if ((long long)blockIdx.x * f.R * RS_TILE >= n_out) return;  // (beyond the row's outputs: nothing is staged)
  polyphase_tiles<LDS_TAPS>(f, n_out, p0, d0, RingSource{src, col0, J, n_in}, RingSink{out, wpos, m.ring_len});
}

// a row with a bad rate index, or with more outputs than the launch was shaped for at its rate, writes nothing
__global__ __launch_bounds__(256) void jitter_release_kernel(JitterRatesArgs m) {
  int ri;
  const int* h = jitter_row(m, ri);
  if (ri < 0 || ri >= m.nr || h[3] > m.r[ri].max_out) return;
  const PolyFilter f = m.r[ri].f;
  if (!f.taps) jitter_release_row<true, false>(m, f, m.r[ri].J, h);
  else if (m.r[ri].lds_taps) jitter_release_row<false, true>(m, f, m.r[ri].J, h);
  else jitter_release_row<false, false>(m, f, m.r[ri].J, h);
}

enum JitterVerb { JIT_PLACE, JIT_CONCEAL, JIT_RELEASE, JIT_NOISE };

// a refusal in the name of the entry point `who` (the jitter and the gate launch cores)
static const char* launch_msg(const char* who, const char* what) {
  static thread_local char msg[160];
  snprintf(msg, sizeof msg, "%s: %s", who, what);
  return msg;
}

// what every verb refuses of one entry of a rate table (ring_fit: how the entry point calls a J outside 1..Js)
static const char* jitter_rate_refusal(const char* who, const JitterRateDesc& d, int Js, const char* ring_fit) {
  if (d.L <= 0 || d.M <= 0 || d.T <= 0) return launch_msg(who, "bad filter shape");
  if (d.taps == nullptr && (d.L != 1 || d.M != 1 || d.T != 1))
    return launch_msg(who, "bad filter shape (no taps is the identity, L = M = T = 1)");
  if (d.J <= 0 || d.J > Js) return launch_msg(who, ring_fit);
  if (d.T - 1 > d.J) return launch_msg(who, "the filter history must fit the rate's ring");
  return nullptr;
}

// The launch of a verb for the entry point `who`: every check (a refusal carries who's name, and nothing is launched), the rate
// table as the kernels take it, the grid.  m comes with the verb's buffers, S, Js, ring_len, mode and the row layout set.
// most: place / conceal: one int, the largest row of the launch; release: per rate the largest n_out (n_rates ints).
static const char* jitter_launch(const char* who, JitterVerb verb, JitterRatesArgs m, const JitterRateDesc* rates, int n_rates,
                                 int rows, const int* most, hipStream_t s) {
  const bool repeat = verb == JIT_CONCEAL && m.mode == 1;
  const char* fit = verb == JIT_PLACE || verb == JIT_NOISE ? "a row's samples must fit its slot's ring"
                  : verb == JIT_CONCEAL ? "a row's samples and its source must fit the ring" : "a row's outputs must fit its slot's ring";
  if (verb == JIT_CONCEAL && m.mode != 0 && m.mode != 1) return launch_msg(who, "mode 0 (zero) or 1 (repeat)");
  if (verb == JIT_PLACE && m.hdr_ints == JIT_PLACE_HDR && (m.enc < 0 || m.enc > 3))
    return launch_msg(who, "encoding 0 (pcm_f32le), 1 (pcm_s16le), 2 (mulaw) or 3 (alaw)");
  if (n_rates < 1 || n_rates > JIT_MAX_RATES) return launch_msg(who, "1 to 16 rates");
  if (!rates) return launch_msg(who, "null rate table");
  if (!most) return launch_msg(who, "null output counts");
  if (!m.hdr || !m.jring || (verb == JIT_PLACE && (!m.stage || m.stage_bytes <= 0)) || (verb == JIT_RELEASE && !m.ring))
    return launch_msg(who, verb == JIT_PLACE ? "null staging buffer, header table or ring" : "null ring or header table");
  if (verb == JIT_NOISE && !m.amp) return launch_msg(who, "null amplitude table");
  if (rows <= 0 || rows > 65535) return launch_msg(who, "1 to 65535 rows");
  // (a launch without rate indices has one rate whose ring is the whole row: a bad J there is a row that does not fit)
  const char* ring_fit = m.rated ? "a rate's ring must fit the ring's rows (1 <= J <= Js)" : fit;
  if (m.Js <= 0) return launch_msg(who, ring_fit);
  if (m.S <= 0 || (verb == JIT_RELEASE ? m.ring_len <= 0 : most[0] < 0)) return launch_msg(who, fit);
  bool fits = false;  // place / conceal: some rate can hold the largest row
  long long gx = 0;   // release: the largest grid and dynamic LDS over the rates present
  size_t lds = 0;
  for (int i = 0; i < n_rates; ++i) {
    const JitterRateDesc& d = rates[i];
    if (const char* bad = jitter_rate_refusal(who, d, m.Js, ring_fit)) return bad;
    const bool ident = d.taps == nullptr;
    if (repeat && (!d.fade || d.P <= 0 || d.F < 0)) return launch_msg(who, "repeat needs a fade table, a period and a fade length");
    JitterRate& r = m.r[i];
    r.f = PolyFilter{d.taps, d.L, d.M, d.T, 0, 0};
    r.fade = d.fade; r.J = d.J; r.P = repeat ? d.P : 0; r.F = repeat ? d.F : 0;
    r.max_out = verb == JIT_RELEASE && most[i] > 0 ? most[i] : 0;
    PolyGrid g;
    if (!poly_grid(r.f, ident, r.max_out, g)) return launch_msg(who, "input / output ratio above 12");
    r.lds_taps = g.lds_taps;
    if (verb != JIT_RELEASE) {
      fits = fits || (long long)most[0] + r.P <= d.J;
    } else {
      if (most[i] < 0 || most[i] > m.ring_len) return launch_msg(who, fit);
      if (r.max_out > 0) {
        gx = g.gx > gx ? g.gx : gx;
        lds = g.lds > lds ? g.lds : lds;
      }
    }
  }
  m.nr = n_rates;
  if (verb != JIT_RELEASE) {
    if (!fits) return launch_msg(who, fit);
    gx = min((most[0] + 255) / 256, 64);
  }
  if (gx == 0) return nullptr;  // no samples to place or conceal, no outputs to release
  const dim3 grid((unsigned)gx, rows);
  if (verb == JIT_PLACE) hipLaunchKernelGGL(jitter_place_kernel, grid, dim3(256), 0, s, m);
  else if (verb == JIT_CONCEAL) hipLaunchKernelGGL(jitter_conceal_kernel, grid, dim3(256), 0, s, m);
  else if (verb == JIT_NOISE) hipLaunchKernelGGL(jitter_noise_kernel, grid, dim3(256), 0, s, m);
  else hipLaunchKernelGGL(jitter_release_kernel, grid, dim3(256), lds, s, m);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

static const char* jitter_place_launch(const char* who, const void* stage, long long stage_bytes, const int* hdr, int hdr_ints, int rows,
                                       int max_n, int enc, const JitterRateDesc* rates, int n_rates, float* jring, int S, int Js,
                                       hipStream_t s) {
  JitterRatesArgs m{};
  m.stage = (const unsigned char*)stage; m.stage_bytes = stage_bytes; m.hdr = hdr; m.jring = jring; m.S = S; m.Js = Js;
  m.hdr_ints = hdr_ints; m.enc = enc; m.rated = hdr_ints == JIT_PLACE_RATES_HDR;
  return jitter_launch(who, JIT_PLACE, m, rates, n_rates, rows, &max_n, s);
}

static const char* jitter_conceal_launch(const char* who, float* jring, int S, int Js, const int* hdr, int hdr_ints, int rows, int max_n,
                                         const JitterRateDesc* rates, int n_rates, int mode, hipStream_t s) {
  JitterRatesArgs m{};
  m.hdr = hdr; m.jring = jring; m.S = S; m.Js = Js; m.mode = mode;
  m.hdr_ints = hdr_ints; m.rated = hdr_ints == JIT_CONCEAL_RATES_HDR;
  return jitter_launch(who, JIT_CONCEAL, m, rates, n_rates, rows, &max_n, s);
}

static const char* jitter_release_launch(const char* who, const float* jring, int S, int Js, const int* hdr, bool rated, int rows,
                                         const JitterRateDesc* rates, int n_rates, const int* max_out, float* ring, int ring_len,
                                         hipStream_t s) {
  JitterRatesArgs m{};
  m.hdr = hdr; m.jring = const_cast<float*>(jring); m.ring = ring; m.S = S; m.Js = Js; m.ring_len = ring_len;
  m.hdr_ints = JIT_RELEASE_HDR; m.rated = rated;
  return jitter_launch(who, JIT_RELEASE, m, rates, n_rates, rows, max_out, s);
}

static const char* jitter_noise_launch(const char* who, float* jring, int S, int Js, const int* hdr, int hdr_ints, int rows, int max_n,
                                       const JitterRateDesc* rates, int n_rates, unsigned seed, const float* amp, hipStream_t s) {
  JitterRatesArgs m{};
  m.hdr = hdr; m.jring = jring; m.S = S; m.Js = Js; m.seed = seed; m.amp = amp;
  m.hdr_ints = hdr_ints; m.rated = hdr_ints == JIT_NOISE_RATES_HDR;
  return jitter_launch(who, JIT_NOISE, m, rates, n_rates, rows, &max_n, s);
}

// the one-rate entry points: a table of one entry built from their scalar arguments, Js = J, rows without a rate index
const char* launch_jitter_place(const void* stage, long long stage_bytes, const int* hdr, int rows, int max_n, int enc,
                                float* jring, int S, int J, hipStream_t s) {
  const JitterRateDesc one{nullptr, nullptr, 1, 1, 1, J, 0, 0};
  return jitter_place_launch("jitter_place", stage, stage_bytes, hdr, JIT_PLACE_HDR, rows, max_n, enc, &one, 1, jring, S, J, s);
}

const char* launch_jitter_place_mixed(const void* stage, long long stage_bytes, const int* hdr, int rows, int max_n, float* jring,
                                      int S, int J, hipStream_t s) {
  const JitterRateDesc one{nullptr, nullptr, 1, 1, 1, J, 0, 0};
  return jitter_place_launch("jitter_place_mixed", stage, stage_bytes, hdr, JIT_PLACE_MIXED_HDR, rows, max_n, 0, &one, 1,
                             jring, S, J, s);
}

const char* launch_jitter_conceal(float* jring, int S, int J, const int* hdr, int rows, int max_n, const float* fade, int P,
                                  int F, int mode, hipStream_t s) {
  const JitterRateDesc one{nullptr, fade, 1, 1, 1, J, P, F};
  return jitter_conceal_launch("jitter_conceal", jring, S, J, hdr, JIT_CONCEAL_HDR, rows, max_n, &one, 1, mode, s);
}

const char* launch_jitter_release(const float* jring, int S, int J, const int* hdr, int rows, int max_out, const float* taps,
                                  int L, int M, int T, float* ring, int ring_len, hipStream_t s) {
  const JitterRateDesc one{taps, nullptr, L, M, T, J, 0, 0};
  return jitter_release_launch("jitter_release", jring, S, J, hdr, false, rows, &one, 1, &max_out, ring, ring_len, s);
}

const char* launch_jitter_noise(float* jring, int S, int J, const int* hdr, int rows, int max_n, unsigned seed, const float* amp,
                                hipStream_t s) {
  const JitterRateDesc one{nullptr, nullptr, 1, 1, 1, J, 0, 0};
  return jitter_noise_launch("jitter_noise", jring, S, J, hdr, JIT_NOISE_HDR, rows, max_n, &one, 1, seed, amp, s);
}

// the _rates entry points: the caller's table, rows that end in their rate index
const char* launch_jitter_noise_rates(float* jring, int S, int Js, const int* hdr, int rows, int max_n, const JitterRateDesc* rates,
                                      int n_rates, unsigned seed, const float* amp, hipStream_t s) {
  return jitter_noise_launch("jitter_noise_rates", jring, S, Js, hdr, JIT_NOISE_RATES_HDR, rows, max_n, rates, n_rates, seed, amp, s);
}

const char* launch_jitter_place_rates(const void* stage, long long stage_bytes, const int* hdr, int rows, int max_n,
                                      const JitterRateDesc* rates, int n_rates, float* jring, int S, int Js, hipStream_t s) {
  return jitter_place_launch("jitter_place_rates", stage, stage_bytes, hdr, JIT_PLACE_RATES_HDR, rows, max_n, 0, rates,
                             n_rates, jring, S, Js, s);
}

const char* launch_jitter_conceal_rates(float* jring, int S, int Js, const int* hdr, int rows, int max_n, const JitterRateDesc* rates,
                                        int n_rates, int mode, hipStream_t s) {
  return jitter_conceal_launch("jitter_conceal_rates", jring, S, Js, hdr, JIT_CONCEAL_RATES_HDR, rows, max_n, rates, n_rates, mode, s);
}

const char* launch_jitter_release_rates(const float* jring, int S, int Js, const int* hdr, int rows, const JitterRateDesc* rates,
                                        int n_rates, const int* max_out, float* ring, int ring_len, hipStream_t s) {
  return jitter_release_launch("jitter_release_rates", jring, S, Js, hdr, true, rows, rates, n_rates, max_out, ring, ring_len, s);
}

// ---------------------------------------------------------------------------------
// Pitch-period concealment (conceal="pitch_sync"; the function is stated in include/afx.h afx_k_jitter_pitch): a released gap
// repeats the last PITCH PERIOD p* of E instead of a fixed 10 ms.  Two verbs beside the four above, on the same ring and under
// the same sizing invariant (lookback >= Pmax + max(Wc, G)):
//   pitch:          one workgroup per gap whose origin a is released now.  The Lh = Pmax + Wc samples before a are quantised to
//                   16-bit integers into LDS; thread t takes the lags Pmin + t, Pmin + t + 256, ...: c(p) and e(p) are exact
//                   integer sums (64-bit accumulation of 32-bit products: any order gives the same numbers), the score
//                   s = c*c / e one fp64 multiply and one IEEE fp64 divide.  The window element q[j] is one LDS address for the
//                   whole wave (a broadcast), q[j - p] consecutive 16-bit words across lanes.  The argmax over the total order
//                   (s descending, p ascending) is a shuffle reduction per wave and the four wave results through LDS.  p*
//                   goes to period[slot]: device state, never read back.
//   conceal_period: jitter_conceal_row with the period read from period[slot] (outside [Pmin, Pmax]: P0) and a gain table of
//                   G = Hd + F entries (1 for Hd samples, then the fade).
// The lag parameters of a rate travel by value beside the rates, as they do.
// ---------------------------------------------------------------------------------
constexpr int JIT_PITCH_HDR = 2, JIT_PITCH_RATES_HDR = 3;  // pitch: slot, ring column of the gap origin a [, rate index]

struct JitterLag {
  const float* gain;             // (max(G, 1),) fp32 (conceal_period only)
  int J, Pmin, Pmax, Wc, P0, G;
};

struct JitterLagArgs {
  const int* hdr;                // (rows, hdr_ints)
  float* jring;                  // (S, Js)
  int* period;                   // (S,)
  int S, Js, nr, hdr_ints, rated;
  JitterLag r[JIT_MAX_RATES];
};

// x -> the 16-bit integer the search runs on: one fp32 multiply, NaN -> 0, round to nearest even, clamp
__device__ __forceinline__ int jitter_quant(float x) {
  const float y = x * 32768.f;
  return y != y ? 0 : (int)fminf(fmaxf(rintf(y), -32768.f), 32767.f);
}

// (s, p) a is before b in the order "s descending, p ascending"; s < 0: no candidate (after every candidate)
__device__ __forceinline__ bool pitch_before(double sa, int pa, double sb, int pb) { return sa > sb || (sa == sb && pa < pb); }

__global__ __launch_bounds__(256) void jitter_pitch_kernel(JitterLagArgs m) {
  extern __shared__ short pitch_q[];  // the Lh quantised samples before a: pitch_q[k] = q[a - Lh + k]
  __shared__ double wave_s[4];
  __shared__ int wave_p[4];
  const int* h = m.hdr + (long long)blockIdx.y * m.hdr_ints;
  const int ri = m.rated ? __builtin_amdgcn_readfirstlane(h[m.hdr_ints - 1]) : 0;
  if (ri < 0 || ri >= m.nr) return;
  const JitterLag& r = m.r[ri];
  const int slot = h[0], ac = h[1], J = r.J, Pmin = r.Pmin, Pmax = r.Pmax, Wc = r.Wc, Lh = Pmax + Wc;
  if (!(slot >= 0 && slot < m.S && ac >= 0 && ac < J && Lh <= J)) return;  // (uniform over the workgroup)
  const float* row = m.jring + (long long)slot * m.Js;
  for (int k = threadIdx.x; k < Lh; k += blockDim.x) {
    int c = ac - Lh + k;  // >= -J
    c = c < 0 ? c + J : c;
    pitch_q[k] = (short)jitter_quant(row[c]);
  }
  __syncthreads();
  double best_s = -1.0;
  int best_p = 0x7fffffff;
  const short* win = pitch_q + Pmax;  // win[t] = q[a - Wc + t]
  for (int p = Pmin + (int)threadIdx.x; p <= Pmax; p += blockDim.x) {
    long long c = 0, e = 0;
    for (int t = 0; t < Wc; ++t) {
      const int x = win[t], y = win[t - p];
      c += (long long)(x * y);
      e += (long long)(y * y);
    }
    if (c > 0 && e > 0) {
      const double s = ((double)c * (double)c) / (double)e;
      if (pitch_before(s, p, best_s, best_p)) { best_s = s; best_p = p; }
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    const double s = __shfl_down(best_s, off, 64);
    const int p = __shfl_down(best_p, off, 64);
    if (pitch_before(s, p, best_s, best_p)) { best_s = s; best_p = p; }
  }
  if ((threadIdx.x & 63) == 0) { wave_s[threadIdx.x >> 6] = best_s; wave_p[threadIdx.x >> 6] = best_p; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w)
      if (pitch_before(wave_s[w], wave_p[w], best_s, best_p)) { best_s = wave_s[w]; best_p = wave_p[w]; }
    m.period[slot] = best_s < 0.0 ? r.P0 : best_p;
  }
}

// jitter_conceal_row in mode 1 with the row's period from period[slot]: E[a + d] = gain[d] * E[a - p + d mod p] for d < G, else 0.
// p is inside [Pmin, Pmax] (a stored value outside it is read as P0), so the source stays inside [a - Pmax, a), disjoint from the
// written columns for d_hi + Pmax <= J.
__global__ __launch_bounds__(256) void jitter_conceal_period_kernel(JitterLagArgs m) {
  const int* h = m.hdr + (long long)blockIdx.y * m.hdr_ints;
  const int ri = m.rated ? __builtin_amdgcn_readfirstlane(h[m.hdr_ints - 1]) : 0;
  if (ri < 0 || ri >= m.nr) return;
  const JitterLag& r = m.r[ri];
  const int slot = h[0], ac = h[1], lo = h[2], hi = h[3], J = r.J, G = r.G;
  if (!(slot >= 0 && slot < m.S && ac >= 0 && ac < J && lo >= 0 && hi >= lo && (long long)hi + r.Pmax <= J)) return;
  int P = m.period[slot];
  P = P < r.Pmin || P > r.Pmax ? r.P0 : P;
  float* row = m.jring + (long long)slot * m.Js;
  const int src0 = ac >= P ? ac - P : ac - P + J;
  for (int d = lo + blockIdx.x * blockDim.x + threadIdx.x; d < hi; d += gridDim.x * blockDim.x) {
    float v = 0.f;
    if (d < G) {
      const int c = src0 + d % P;
      v = r.gain[d] * row[c < J ? c : c - J];
    }
    const int w = ac + d;  // < 2 J
    row[w < J ? w : w - J] = v;
  }
}

// The launch of the two verbs for the entry point `who`: the estimate (one workgroup per row; max_n is not read) or the synthesis
// (max_n = the largest d_hi - d_lo).  Every check first; a refusal carries who's name, and nothing is launched.
static const char* jitter_lag_launch(const char* who, bool estimate, float* jring, int S, int Js, const int* hdr, int hdr_ints, bool rated,
                                     int rows, int max_n, const JitterRateDesc* rates, const JitterLagDesc* lags, int n_rates,
                                     int* period, hipStream_t s) {
  if (n_rates < 1 || n_rates > JIT_MAX_RATES) return launch_msg(who, "1 to 16 rates");
  if (!rates || !lags) return launch_msg(who, "null rate table");
  if (!hdr || !jring || !period) return launch_msg(who, "null ring, header table or period state");
  if (rows <= 0 || rows > 65535) return launch_msg(who, "1 to 65535 rows");
  const char* ring_fit = rated ? "a rate's ring must fit the ring's rows (1 <= J <= Js)"
                       : estimate ? "the search history Pmax + Wc must fit a rate's ring" : "a row's samples and its source must fit the ring";
  const char* rows_fit = "a row's samples and its source must fit the ring";
  if (Js <= 0 || S <= 0 || (!estimate && max_n < 0)) return launch_msg(who, Js <= 0 ? ring_fit : rows_fit);
  JitterLagArgs m{};
  m.hdr = hdr; m.jring = jring; m.period = period; m.S = S; m.Js = Js; m.nr = n_rates; m.hdr_ints = hdr_ints; m.rated = rated;
  bool fits = false;  // some rate can hold the history (estimate) or the largest row and its source (synthesis)
  int lh = 0;         // estimate: the longest history among the rates that hold theirs
  for (int i = 0; i < n_rates; ++i) {
    const JitterRateDesc& d = rates[i];
    const JitterLagDesc& g = lags[i];
    if (const char* bad = jitter_rate_refusal(who, d, Js, ring_fit)) return bad;
    if (g.Pmin < 1) return launch_msg(who, "the shortest lag Pmin must be at least 1");
    if (g.Pmax < g.Pmin) return launch_msg(who, "the longest lag Pmax must not be below Pmin");
    if (g.Wc < 1) return launch_msg(who, "the correlation window Wc must be at least 1");
    if (g.P0 < g.Pmin || g.P0 > g.Pmax) return launch_msg(who, "the fallback period P0 must lie in [Pmin, Pmax]");
    if (!estimate && (!d.fade || g.Hd < 0 || d.F < 0)) return launch_msg(who, "synthesis needs a gain table, a hold and a fade length");
    m.r[i] = JitterLag{d.fade, d.J, g.Pmin, g.Pmax, g.Wc, g.P0, estimate ? 0 : g.Hd + d.F};
    const long long Lh = (long long)g.Pmax + g.Wc;
    if (estimate ? Lh <= d.J : (long long)max_n + g.Pmax <= d.J) {
      fits = true;
      lh = Lh > lh ? (int)Lh : lh;
    } else if (estimate) {
      m.r[i].J = 0;  // (a rate whose ring cannot hold its history: every row of it is skipped, whatever Lh is as an int)
    }
  }
  if (!fits) return launch_msg(who, estimate ? "the search history Pmax + Wc must fit a rate's ring" : rows_fit);
  if (estimate) {
    if (lh > 32000) return launch_msg(who, "the search history Pmax + Wc must fit 64 KB of LDS as 16-bit samples");
    hipLaunchKernelGGL(jitter_pitch_kernel, dim3(1, rows), dim3(256), (size_t)lh * sizeof(short), s, m);
  } else {
    const int gx = min((max_n + 255) / 256, 64);
    if (gx == 0) return nullptr;  // no samples to conceal
    hipLaunchKernelGGL(jitter_conceal_period_kernel, dim3(gx, rows), dim3(256), 0, s, m);
  }
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

const char* launch_jitter_pitch(const float* jring, int S, int J, const int* hdr, int rows, int Pmin, int Pmax, int Wc, int P0,
                                int* period, hipStream_t s) {
  const JitterRateDesc one{nullptr, nullptr, 1, 1, 1, J, 0, 0};
  const JitterLagDesc lag{Pmin, Pmax, Wc, P0, 0};
  return jitter_lag_launch("jitter_pitch", true, const_cast<float*>(jring), S, J, hdr, JIT_PITCH_HDR, false, rows, 0, &one, &lag, 1, period, s);
}

const char* launch_jitter_pitch_rates(const float* jring, int S, int Js, const int* hdr, int rows, const JitterRateDesc* rates,
                                      const JitterLagDesc* lags, int n_rates, int* period, hipStream_t s) {
  return jitter_lag_launch("jitter_pitch_rates", true, const_cast<float*>(jring), S, Js, hdr, JIT_PITCH_RATES_HDR, true, rows, 0, rates, lags,
                           n_rates, period, s);
}

const char* launch_jitter_conceal_period(float* jring, int S, int J, const int* hdr, int rows, int max_n, const float* gain,
                                         const int* period, int Pmin, int Pmax, int P0, int Hd, int F, hipStream_t s) {
  const JitterRateDesc one{nullptr, gain, 1, 1, 1, J, P0, F};
  const JitterLagDesc lag{Pmin, Pmax, 1, P0, Hd};  // (the synthesis reads no correlation window)
  return jitter_lag_launch("jitter_conceal_period", false, jring, S, J, hdr, JIT_CONCEAL_HDR, false, rows, max_n, &one, &lag, 1,
                           const_cast<int*>(period), s);
}

const char* launch_jitter_conceal_period_rates(float* jring, int S, int Js, const int* hdr, int rows, int max_n,
                                               const JitterRateDesc* rates, const JitterLagDesc* lags, int n_rates, const int* period,
                                               hipStream_t s) {
  return jitter_lag_launch("jitter_conceal_period_rates", false, jring, S, Js, hdr, JIT_CONCEAL_RATES_HDR, true, rows, max_n, rates, lags,
                           n_rates, const_cast<int*>(period), s);
}

// ---------------------------------------------------------------------------------
// Speech gate (afx/vad.py; the function is stated in include/afx.h afx_k_gate): a per-slot energy gate over frames of
// `frame` 16 kHz samples with a tracked noise floor and a hangover; the kept frames of a row are compacted, bit for bit, into
// the slot's pending ring (the layout ingest_pop_kernel reads).  The gate has three forms -- plain (gate_kernel), with onset
// look-ahead (gate_la_kernel) and with call-tone rejection (gate_tone_kernel) -- and each kernel is a composition of the
// phases below, every shared phase written once.  One workgroup per row:
//   guard     gate_row: slot and wpos from the header; a row that fails a condition writes nothing but kept = 0;
//   energies  gate_energies: the four waves compute the frame energies into LDS: lane l sums sq[l], sq[l + 64], ... in
//             ascending order, then a shuffle-down tree folds the 64 partials (w = 32 .. 1).  Every operation is one
//             correctly rounded fp32 multiply or add (contraction is off in gate_frame_energy: p + v * v must not become
//             an fma), so numpy float32 restates it;
//   decision  thread 0 runs the state machine over the frames in stream order (a serial recurrence of a few ops per
//             frame): gate_speech (speech, and the floor update), the form's own lines, gate_keep (hangover and keep),
//             then each frame's offset among the samples the launch keeps (or -1: dropped) to LDS;
//   epilogue  gate_store: nf, h and kept (accumulated over the launches of a row) to device memory;
//   copy      gate_copy_kept: the four waves copy the kept frames, 64 consecutive samples per step (plain and tone; the
//             look-ahead kernel copies out of its delay line and has a copy of its own).
// The helpers hold no barrier: every __syncthreads() stands in a kernel body, between the phases it separates.
// A launch takes at most GATE_MAX_FRAMES frames of a row (what its LDS tables hold); gate_launch splits a longer row into
// successive launches that find nf, h and the samples kept so far in device memory.
// ---------------------------------------------------------------------------------
constexpr int GATE_MAX_FRAMES = 512;  // frames of a row per launch: 2 x 512 x 4 bytes of LDS (include/afx.h states it)

// What the three forms share; GateLaArgs and GateToneArgs hold one and add their own fields.  100 bytes without tail
// padding (hence the attribute), so that the look-ahead kernel's arguments fill the 128 bytes they always did: a kernel
// reads its arguments from memory with scalar loads that the compiler places where it likes, some of them late, and with
// one more line of arguments such a load can miss on its own (profiles/gate_refactor_ab.txt has both layouts).
struct __attribute__((packed, aligned(4))) GateArgs {
  const float* x;    // (A, n) samples, row i = the next n samples of slot hdr[i][0]
  const int* hdr;    // (A, 2 or 4): slot, wpos, then the form's own columns
  float* nf;         // (S,) noise floor per slot
  int* h;            // (S,) hangover frames left per slot
  float* ring;       // (S, ring_len)
  int* kept;         // (A,) samples kept (look-ahead: emitted) of each row
  unsigned char* mask;  // (A, n / frame) per frame, what the form states, or nullptr
  int n, frame, f0, nframes;  // this launch: frames [f0, f0 + nframes) of the n / frame of a row
  int S, ring_len, hang;
  float e_floor, ratio, rise, nf_min;
};

// the energy of one frame as lane `lane` of a wave sees it (lane 0 holds the result)
__device__ __forceinline__ float gate_frame_energy(const float* __restrict__ x, int frame, int lane) {
#pragma clang fp contract(off)
  float p = 0.f;
  if (lane < frame) {
    const float v = x[lane];
    p = v * v;
  }
  for (int i = lane + 64; i < frame; i += 64) {
    const float v = x[i];
    const float sq = v * v;
    p = p + sq;
  }
  for (int w = 32; w >= 1; w >>= 1) {
    const float q = __shfl_down(p, w);  // lanes l < w take p[l + w]: the lanes the next step reads
    p = p + q;
  }
  return p;
}

// guard: slot and wpos of the row from its header of hdr_ints columns, and whether the row is gated: the conditions of
// every form and `own`, the calling form's.  A row that fails writes nothing but kept = 0, once (at the first launch of a
// split row).
__device__ __forceinline__ bool gate_row(const GateArgs& g, int row, int tid, int hdr_ints, bool own, int& slot, int& wpos) {
  slot = g.hdr[hdr_ints * row];
  wpos = g.hdr[hdr_ints * row + 1];
  if (own && slot >= 0 && slot < g.S && wpos >= 0 && wpos < g.ring_len && g.n <= g.ring_len) return true;
  if (tid == 0 && g.f0 == 0) g.kept[row] = 0;
  return false;
}

// the launch's first sample of the row
__device__ __forceinline__ const float* gate_row_x(const GateArgs& g, int row) {
  return g.x + (long long)row * g.n + (long long)g.f0 * g.frame;
}

// energies: the frames of the launch (x: the first) to s_e, a frame per wave and step
__device__ __forceinline__ void gate_energies(const GateArgs& g, const float* __restrict__ x, int wave, int lane, float* s_e) {
  for (int f = wave; f < g.nframes; f += 4) {
    const float e = gate_frame_energy(x + (long long)f * g.frame, g.frame, lane);
    if (lane == 0) s_e[f] = e;
  }
}

// decision, first half: is the frame of energy e speech against the floor nf, and the floor's update
__device__ __forceinline__ bool gate_speech(const GateArgs& g, float e, float& nf) {
#pragma clang fp contract(off)
  const bool fin = e < INFINITY;  // (false for a NaN too)
  const bool speech = fin && e > fmaxf(g.e_floor, g.ratio * nf);
  if (fin) nf = fmaxf(g.nf_min, fminf(e, nf * g.rise));
  return speech;
}

// decision, second half: the hangover h and whether the frame is kept.  (Two halves: between them the tone gate
// takes speech and the hangover away from a tone frame.)
__device__ __forceinline__ bool gate_keep(const GateArgs& g, bool speech, int& h) {
#pragma clang fp contract(off)
  if (speech) h = g.hang;
  const bool keep = speech || h > 0;
  if (!speech && h > 0) --h;
  return keep;
}

// epilogue (thread 0): the slot's state, the row's count over the launches so far, and the count before this launch for the copy
__device__ __forceinline__ void gate_store(const GateArgs& g, int slot, int row, float nf, int h, int off, int* s_base) {
  const int base = g.f0 ? g.kept[row] : 0;
  g.nf[slot] = nf;
  g.h[slot] = h;
  g.kept[row] = base + off;
  *s_base = base;
}

// one frame, 64 consecutive samples per step, where neither side wraps
__device__ __forceinline__ void gate_copy_frame(float* __restrict__ to, const float* __restrict__ from, int frame, int lane) {
  for (int k = lane; k < frame; k += 64) to[k] = from[k];
}

// copy: the frames with an offset in s_off from x into the slot's ring behind wpos + base, a frame per wave and step
__device__ __forceinline__ void gate_copy_kept(const GateArgs& g, const float* __restrict__ x, int slot, int wpos, int base,
                                               const int* s_off, int wave, int lane) {
  float* out = g.ring + (long long)slot * g.ring_len;
  const long long w0 = (long long)wpos + base;  // base + off + k < n <= ring_len: one wrap
  for (int f = wave; f < g.nframes; f += 4) {
    const int off = s_off[f];
    if (off < 0) continue;
    const float* src = x + (long long)f * g.frame;
    for (int k = lane; k < g.frame; k += 64) {
      const long long w = w0 + off + k;
      out[w < g.ring_len ? w : w - g.ring_len] = src[k];
    }
  }
}

__global__ __launch_bounds__(256) void gate_kernel(GateArgs a) {
  __shared__ float s_e[GATE_MAX_FRAMES];
  __shared__ int s_off[GATE_MAX_FRAMES];  // offset of the frame among this launch's kept samples, -1: dropped
  __shared__ int s_base;                  // samples of the row kept by the launches before this one
  const int row = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  int slot, wpos;
  if (!gate_row(a, row, tid, 2, true, slot, wpos)) return;
  const float* x = gate_row_x(a, row);
  gate_energies(a, x, wave, lane, s_e);
  __syncthreads();
  if (tid == 0) {
    float nf = a.nf[slot];
    int h = a.h[slot], off = 0;
    for (int f = 0; f < a.nframes; ++f) {
      const bool speech = gate_speech(a, s_e[f], nf);
      const bool keep = gate_keep(a, speech, h);
      s_off[f] = keep ? off : -1;
      if (keep) off += a.frame;
      if (a.mask) a.mask[(long long)row * (a.n / a.frame) + a.f0 + f] = keep;
    }
    gate_store(a, slot, row, nf, h, off, &s_base);
  }
  __syncthreads();
  gate_copy_kept(a, x, slot, wpos, s_base, s_off, wave, lane);
}

// The launch of a form for the entry point `who`: the checks the forms share (a refusal carries who's name, and nothing is
// launched), nf_min, and one launch per GATE_MAX_FRAMES frames of a row.  g comes with the buffers, shapes and constants
// set; launch(g) launches the form's kernel over g with f0 and nframes set.  The form's own checks are its launcher's.
template <class Launch>
static const char* gate_launch(const char* who, GateArgs g, int A, Launch launch) {
  if (!g.x || !g.hdr || !g.nf || !g.h || !g.ring || !g.kept) return launch_msg(who, "null argument");
  if (A <= 0 || A > 65535) return launch_msg(who, "1 to 65535 rows");
  if (g.frame <= 0 || g.n <= 0 || g.n % g.frame) return launch_msg(who, "a row is a positive whole number of frames");
  if (g.S <= 0 || g.ring_len <= 0) return launch_msg(who, "no slots or no ring");
  if (!(g.e_floor > 0.f && g.e_floor < INFINITY && g.ratio > 1.f && g.ratio < INFINITY && g.rise >= 1.f && g.rise < INFINITY) ||
      g.hang < 0)
    return launch_msg(who, "floor > 0, ratio > 1, rise >= 1 (all finite) and hang >= 0");
  g.nf_min = g.e_floor / g.ratio;  // (one IEEE fp32 division, on the host)
  const int frames = g.n / g.frame;
  for (g.f0 = 0; g.f0 < frames; g.f0 += GATE_MAX_FRAMES) {
    g.nframes = min(GATE_MAX_FRAMES, frames - g.f0);
    launch(g);
  }
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

// the arguments every form's entry point takes, as the kernels take them
static GateArgs gate_args(const float* x, int n, const int* hdr, int frame, float e_floor, float ratio, float rise, int hang,
                          float* nf, int* h, float* ring, int S, int ring_len, int* kept, unsigned char* mask) {
  GateArgs g{};
  g.x = x; g.hdr = hdr; g.nf = nf; g.h = h; g.ring = ring; g.kept = kept; g.mask = mask;
  g.n = n; g.frame = frame; g.S = S; g.ring_len = ring_len; g.hang = hang;
  g.e_floor = e_floor; g.ratio = ratio; g.rise = rise;
  return g;
}

const char* launch_gate(const float* x, int A, int n, const int* hdr, int frame, float e_floor, float ratio, float rise, int hang,
                        float* nf, int* h, float* ring, int S, int ring_len, int* kept, unsigned char* mask, hipStream_t s) {
  return gate_launch("gate", gate_args(x, n, hdr, frame, e_floor, ratio, rise, hang, nf, h, ring, S, ring_len, kept, mask), A,
                     [&](const GateArgs& g) { hipLaunchKernelGGL(gate_kernel, dim3(A), dim3(256), 0, s, g); });
}

// ---------------------------------------------------------------------------------
// Look-ahead gate (afx/vad.py LookaheadGate; the function is stated in include/afx.h afx_k_gate_la): the plain gate's
// decision per frame, behind a delay line of `pre` frames per slot.  Frame G (counted from the slot's reset) enters the line
// with flag = keep; a speech frame flags every frame then in the line; frame G - pre leaves while frame G is processed and
// is emitted into the pending ring iff its flag is set, with its index G - pre recorded in src.  One workgroup per row, the
// shared phases (guard, energies, decision halves, epilogue) and three departures: the guard also wants wpos on the frame
// grid and F with room for the row's frames; between the decision's halves and after them thread 0 keeps the line's flags
// and writes, per frame of the launch, the offset of the frame that LEAVES (-1: none, or dropped); and the copy is this
// kernel's own, because a leaving frame comes out of the line or out of x and its source index goes to src.  Two hazards:
//   block reuse: frame G - pre leaves from the line block (G mod pre) that frame G enters.  A launch therefore copies the
//      leaving frames that an earlier launch stored (the first min(pre, nframes) steps) out of the line, then a barrier,
//      and only then stores its own last min(pre, nframes) frames into the line.  A frame that enters and leaves within one
//      launch is copied from x directly and never touches the line;
//   rows longer than GATE_MAX_FRAMES: gate_launch splits them into successive launches, each complete in itself (it
//      leaves its last frames in the line, flags in flags, nf, h and the samples emitted so far in kept), so the next finds
//      everything in device memory and the result does not depend on the split.
// wpos and ring_len are whole frames, so no frame straddles the ring's wrap.
// ---------------------------------------------------------------------------------
struct GateLaArgs {
  GateArgs g;        // hdr (A, 4): slot, wpos, F (frames the slot was pushed before this row), 0; kept: samples emitted;
                     // mask entry j: keep' of source frame F - pre + j (0 where negative)
  int pre;           // (behind g's 100 bytes, so that the pointers follow without padding)
  int* flags;        // (S,) bit (g mod pre): the flag of delayed frame g
  float* line;       // (S, pre * frame) delayed frame g at block g mod pre
  int* src;          // (S, ring_len / frame) source index of the frame at ring position w, at entry w / frame
};
static_assert(sizeof(GateLaArgs) == 128, "gate_la_kernel's arguments: 128 bytes (see GateArgs)");

__global__ __launch_bounds__(256) void gate_la_kernel(GateLaArgs a) {
  __shared__ float s_e[GATE_MAX_FRAMES];
  __shared__ int s_off[GATE_MAX_FRAMES];  // offset, among this launch's emitted samples, of the frame leaving at step j; -1: none
  __shared__ int s_base;                  // samples of the row emitted by the launches before this one
  const GateArgs& g = a.g;
  const int row = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int F = g.hdr[4 * row + 2], frames = g.n / g.frame;
  int slot, wpos;
  if (!gate_row(g, row, tid, 4, g.hdr[4 * row + 1] % g.frame == 0 && F >= 0 && F <= 0x7fffffff - frames, slot, wpos)) return;
  const int G0 = F + g.f0, pre = a.pre;  // the index of this launch's first frame
  const float* x = gate_row_x(g, row);
  gate_energies(g, x, wave, lane, s_e);
  __syncthreads();
  if (tid == 0) {
    float nf = g.nf[slot];
    int h = g.h[slot], off = 0, b = G0 % pre;  // b = G mod pre: the block frame G enters and frame G - pre leaves
    unsigned fl = (unsigned)a.flags[slot];
    const unsigned all = (1u << pre) - 1u;
    for (int f = 0; f < g.nframes; ++f) {
      const int G = G0 + f;
      const bool speech = gate_speech(g, s_e[f], nf);
      if (speech) fl = G >= pre ? all : (1u << G) - 1u;  // every frame now in the line (blocks not yet filled stay 0)
      const bool out = G >= pre && ((fl >> b) & 1u);
      const bool keep = gate_keep(g, speech, h);
      fl = (fl & ~(1u << b)) | ((unsigned)keep << b);  // frame G enters with flag = keep
      s_off[f] = out ? off : -1;
      if (out) off += g.frame;
      if (g.mask) g.mask[(long long)row * frames + g.f0 + f] = out;
      b = b + 1 == pre ? 0 : b + 1;
    }
    a.flags[slot] = (int)fl;
    gate_store(g, slot, row, nf, h, off, &s_base);
  }
  __syncthreads();
  float* out = g.ring + (long long)slot * g.ring_len;
  int* so = a.src + (long long)slot * (g.ring_len / g.frame);
  float* ln = a.line + (long long)slot * pre * g.frame;
  const int w0 = wpos + s_base;  // base + off + frame <= n <= ring_len: one wrap, at a frame edge
  const int old = min(pre, g.nframes);  // steps whose leaving frame an earlier launch stored in the line
  for (int f = wave; f < g.nframes; f += 4) {
    const int off = s_off[f];
    if (off < 0) continue;
    const float* from = f < old ? ln + (long long)((G0 + f) % pre) * g.frame : x + (long long)(f - pre) * g.frame;
    const int w = w0 + off < g.ring_len ? w0 + off : w0 + off - g.ring_len;
    gate_copy_frame(out + w, from, g.frame, lane);
    if (lane == 0) so[w / g.frame] = G0 + f - pre;
  }
  __syncthreads();  // every copy out of the line is done before a frame of this launch is stored into it
  for (int f = g.nframes - old + wave; f < g.nframes; f += 4)
    gate_copy_frame(ln + (long long)((G0 + f) % pre) * g.frame, x + (long long)f * g.frame, g.frame, lane);
}

const char* launch_gate_la(const float* x, int A, int n, const int* hdr, int frame, float e_floor, float ratio, float rise,
                           int hang, int pre, float* nf, int* h, int* flags, float* line, float* ring, int* src, int S,
                           int ring_len, int* kept, unsigned char* mask, hipStream_t s) {
  if (!flags || !line || !src) return "gate_la: null argument";
  if (frame > 0 && (S <= 0 || ring_len <= 0 || ring_len > (1 << 30) || ring_len % frame))
    return "gate_la: no slots, or a ring that is not whole frames (at most 2^30 samples)";
  if (pre < 1 || pre > 31) return "gate_la: 1 to 31 frames of pre-roll";
  GateLaArgs a{gate_args(x, n, hdr, frame, e_floor, ratio, rise, hang, nf, h, ring, S, ring_len, kept, mask), pre, flags, line, src};
  return gate_launch("gate_la", a.g, A, [&](const GateArgs& g) {
    a.g = g;
    hipLaunchKernelGGL(gate_la_kernel, dim3(A), dim3(256), 0, s, a);
  });
}

// ---------------------------------------------------------------------------------
// Tone gate (afx/vad.py ToneGate; the function is stated in include/afx.h afx_k_gate_tone): the plain gate's decision plus
// a Goertzel bank of K <= 16 signalling frequencies per frame.  A frame whose two largest bank powers hold at least
// thr * e is `tonal`; `confirm` tonal frames in a row make a tone, which lasts `hold` frames past the run; a tone frame is
// not speech, is not kept and ends the hangover.  One workgroup per row, the plain gate's phases (guard, energies, decision
// halves, epilogue, gate_copy_kept) and two departures:
//   powers    beside the energies, the (frame, k) pairs of the launch are spread over the 256 threads, k fastest (a
//             frame's K lanes read one sample address): each pair runs the second-order recurrence over its frame's
//             samples sequentially, three dependent fp32 operations per sample with contraction off, and leaves its power
//             in LDS; then one thread per frame folds the K powers into T = the sum of the two largest positive ones;
//   decision  between gate_speech and gate_keep thread 0 runs r, q and tones, and a tone frame loses speech and the
//             hangover there; it also writes tsum and counts ntone (which a skipped row zeroes beside kept).
// LDS at GATE_MAX_FRAMES: 3 tables of 512 x 4 bytes and the powers, 512 x 16 x 4 = 32 KB; 38 KB of a workgroup's 64 KB.
// The samples are read eight at a time so that the loads run ahead of the dependent chain.
// ---------------------------------------------------------------------------------
constexpr int GATE_MAX_TONES = 16;  // frequencies of a bank (include/afx.h states it)

struct GateToneArgs {
  GateArgs g;         // hdr (A, 2): slot, wpos; mask: bit 0 keep, bit 1 tone, bit 2 tonal
  const float* coef;  // (K,) 2 cos(2 pi f_k / 16000)
  int* tone_state;    // (S, 3): r (tonal frames in a row), q (hold frames left), tones (tone frames since the reset)
  int* ntone;         // (A,) tone frames of each row, or nullptr
  float* tsum;        // (A, n / frame) T of every frame, or nullptr
  int K, confirm, hold;
  float thr;
};

// the Goertzel power of one frame at the coefficient c: every operation one correctly rounded fp32 multiply, add or subtract
__device__ __forceinline__ float gate_tone_power(const float* __restrict__ x, int frame, float c) {
#pragma clang fp contract(off)
  float s1 = 0.f, s2 = 0.f;
  int i = 0;
  for (; i + 8 <= frame; i += 8) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = x[i + j];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float t = c * s1;
      t = t - s2;
      const float s0 = v[j] + t;
      s2 = s1;
      s1 = s0;
    }
  }
  for (; i < frame; ++i) {
    float t = c * s1;
    t = t - s2;
    const float s0 = x[i] + t;
    s2 = s1;
    s1 = s0;
  }
  const float a = s1 * s1, b = s2 * s2;
  float m = c * s1;
  m = m * s2;
  const float ab = a + b;
  return ab - m;
}

__global__ __launch_bounds__(256) void gate_tone_kernel(GateToneArgs a) {
  __shared__ float s_e[GATE_MAX_FRAMES];
  __shared__ float s_t[GATE_MAX_FRAMES];  // T of the frame
  __shared__ int s_off[GATE_MAX_FRAMES];  // offset of the frame among this launch's kept samples, -1: dropped
  __shared__ float s_p[GATE_MAX_FRAMES * GATE_MAX_TONES];  // power of pair f * K + k
  __shared__ int s_base;                  // samples of the row kept by the launches before this one
  const GateArgs& g = a.g;
  const int row = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  int slot, wpos;
  if (!gate_row(g, row, tid, 2, true, slot, wpos)) {
    if (tid == 0 && g.f0 == 0 && a.ntone) a.ntone[row] = 0;
    return;
  }
  const float* x = gate_row_x(g, row);
  gate_energies(g, x, wave, lane, s_e);
  const int K = a.K;
  for (int p = tid; p < g.nframes * K; p += 256) {  // (nframes * K <= 512 * 16)
    const int f = p / K, k = p - f * K;
    s_p[p] = gate_tone_power(x + (long long)f * g.frame, g.frame, a.coef[k]);
  }
  __syncthreads();
  for (int f = tid; f < g.nframes; f += 256) {
    float p1 = 0.f, p2 = 0.f;  // the two largest positive powers (a NaN or non-positive power counts as +0.0)
    for (int k = 0; k < K; ++k) {
      const float v = s_p[f * K + k];
      if (v > p1) {
        p2 = p1;
        p1 = v;
      } else if (v > p2) {
        p2 = v;
      }
    }
    s_t[f] = p1 + p2;
  }
  __syncthreads();
  if (tid == 0) {
#pragma clang fp contract(off)
    const long long frames = g.n / g.frame;
    float nf = g.nf[slot];
    int h = g.h[slot], off = 0, nt = 0;
    int r = a.tone_state[3 * slot], q = a.tone_state[3 * slot + 1], tones = a.tone_state[3 * slot + 2];
    for (int f = 0; f < g.nframes; ++f) {
      const float e = s_e[f], T = s_t[f];
      bool speech = gate_speech(g, e, nf);
      const float bound = a.thr * e;
      const bool tonal = e < INFINITY && e > g.e_floor && T >= bound;  // (false for a NaN e or T)
      r = tonal ? (r < 0x7fffffff ? r + 1 : r) : 0;
      if (r >= a.confirm) q = a.hold;
      const bool tone = r >= a.confirm || q > 0;
      if (r < a.confirm && q > 0) --q;
      if (tone) {
        if (tones < 0x7fffffff) ++tones;
        ++nt;
        speech = false;
        h = 0;
      }
      const bool keep = gate_keep(g, speech, h);
      s_off[f] = keep ? off : -1;
      if (keep) off += g.frame;
      if (g.mask) g.mask[row * frames + g.f0 + f] = (unsigned char)((keep ? 1 : 0) | (tone ? 2 : 0) | (tonal ? 4 : 0));
      if (a.tsum) a.tsum[row * frames + g.f0 + f] = T;
    }
    a.tone_state[3 * slot] = r;
    a.tone_state[3 * slot + 1] = q;
    a.tone_state[3 * slot + 2] = tones;
    if (a.ntone) a.ntone[row] = (g.f0 ? a.ntone[row] : 0) + nt;
    gate_store(g, slot, row, nf, h, off, &s_base);
  }
  __syncthreads();
  gate_copy_kept(g, x, slot, wpos, s_base, s_off, wave, lane);
}

const char* launch_gate_tone(const float* x, int A, int n, const int* hdr, int frame, float e_floor, float ratio, float rise,
                             int hang, const float* coef, int K, float thr, int confirm, int hold, float* nf, int* h,
                             int* tone_state, float* ring, int S, int ring_len, int* kept, int* ntone, unsigned char* mask,
                             float* tsum, hipStream_t s) {
  if (!coef || !tone_state) return "gate_tone: null argument";
  if (K < 1 || K > GATE_MAX_TONES) return "gate_tone: a bank of 1 to 16 frequencies";
  if (!(thr > 0.f && thr < INFINITY) || confirm < 1 || hold < 0)
    return "gate_tone: thr > 0 (finite), confirm >= 1 and hold >= 0";
  GateToneArgs a{gate_args(x, n, hdr, frame, e_floor, ratio, rise, hang, nf, h, ring, S, ring_len, kept, mask),
                 coef, tone_state, ntone, tsum, K, confirm, hold, thr};
  return gate_launch("gate_tone", a.g, A, [&](const GateArgs& g) {
    a.g = g;
    hipLaunchKernelGGL(gate_tone_kernel, dim3(A), dim3(256), 0, s, a);
  });
}

// ---------------------------------------------------------------------------------
// Talk spurts (afx/turns.py; the function is stated in include/afx.h afx_k_turn / afx_k_turn_collect): behind a gate launch
// that compacted the kept frames of each row into a staging ring and wrote the per-frame mask, turn_kernel cuts each slot's
// stream into turns -- maximal runs of kept frames, cut at max_frames -- and appends the row's kept frames to the slot's open
// turn, in one of two buffers per slot; turn_collect_kernel then tiles the turns the push completed into padded clips.  Both
// are copies: no floating-point arithmetic.  turn_kernel, one workgroup per row, in the gate kernels' phases:
//   guard     slot, wpos and g0 from the header and the slot's state; a row that fails writes done = (-1, -1, -1, -1) only;
//   plan      thread 0 walks the mask in stream order (a serial recurrence of a few integer ops per frame) and writes per
//             frame (staging frame r or -1, destination frame among the slot's 2 x max_frames) to LDS, then state, totals
//             and done.  The frames of a turn the row itself drops as short are taken out of the plan again: the next turn
//             starts at the same place of the same buffer, and two waves must not write one destination;
//   copy      after the barrier the four waves copy a frame per wave and step: 16 bytes per lane where frame, the ring
//             length and wpos are multiples of 4 and both bases are 16-byte aligned (a 4-vector then never straddles the
//             ring's wrap), one sample per lane otherwise.
// ---------------------------------------------------------------------------------
constexpr int TURN_MAX_FRAMES = 512;  // frames of a row: the plan, 512 x 8 bytes of LDS (include/afx.h states it)

struct TurnArgs {
  const float* staging;       // (S, ring_len): the row's kept frames in order from wpos on
  const unsigned char* mask;  // (A, F): bit 0 = kept
  const int* hdr;             // (A, 3): slot, wpos, g0
  float* bufs;                // (S, 2, max_frames * frame)
  int* state;                 // (S, 3): open, n, g
  int* totals;                // (S, 4): scored, short, cut, kept, saturating
  int* done;                  // (A, 4): buffer, frames, first source frame, one past the last
  int S, ring_len, F, frame, min_frames, max_frames, vec;
};

__device__ __forceinline__ int turn_count(int v) { return v < 0x7fffffff ? v + 1 : v; }

__global__ __launch_bounds__(256) void turn_kernel(TurnArgs a) {
  __shared__ int2 s_plan[TURN_MAX_FRAMES];  // x: the staging frame, -1: nothing to copy; y: open * max_frames + n
  const int row = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int slot = a.hdr[3 * row], wpos = a.hdr[3 * row + 1], g0 = a.hdr[3 * row + 2];
  bool ok = slot >= 0 && slot < a.S && wpos >= 0 && wpos < a.ring_len && g0 >= 0 && g0 <= 0x7fffffff - a.F;
  int open = 0, n = 0;
  if (ok) {  // (a state that is not a turn state would leave the buffers: such a row is skipped too)
    open = a.state[3 * slot];
    n = a.state[3 * slot + 1];
    ok = (open == 0 || open == 1) && n >= 0 && n < a.max_frames;
  }
  if (!ok) {
    if (tid < 4) a.done[4 * row + tid] = -1;
    return;
  }
  if (tid == 0) {
    int g = a.state[3 * slot + 2];
    int* tot = a.totals + 4 * slot;
    int scored = tot[0], shrt = tot[1], cut = tot[2], kept = tot[3];
    int d0 = 0, d1 = 0, d2 = 0, d3 = 0, r = 0, j0 = 0;  // j0: the open turn's first frame in this row
    const unsigned char* m = a.mask + (long long)row * a.F;
    for (int j = 0; j < a.F; ++j) {
      const int G = g0 + j;
      if (m[j] & 1) {
        if (n == 0) { g = G; j0 = j; }
        s_plan[j] = make_int2(r, open * a.max_frames + n);
        ++r; ++n;
        kept = turn_count(kept);
        if (n == a.max_frames) {
          d0 = open; d1 = n; d2 = g; d3 = G + 1;
          scored = turn_count(scored); cut = turn_count(cut);
          open ^= 1; n = 0;
        }
      } else {
        s_plan[j] = make_int2(-1, 0);
        if (n > 0) {
          if (n >= a.min_frames) {
            d0 = open; d1 = n; d2 = g; d3 = G;
            scored = turn_count(scored);
            open ^= 1;
          } else {
            shrt = turn_count(shrt);
            for (int k = j0; k < j; ++k) s_plan[k].x = -1;
          }
          n = 0;
        }
      }
    }
    a.state[3 * slot] = open; a.state[3 * slot + 1] = n; a.state[3 * slot + 2] = g;
    tot[0] = scored; tot[1] = shrt; tot[2] = cut; tot[3] = kept;
    a.done[4 * row] = d0; a.done[4 * row + 1] = d1; a.done[4 * row + 2] = d2; a.done[4 * row + 3] = d3;
  }
  __syncthreads();
  const float* src = a.staging + (long long)slot * a.ring_len;
  float* dst = a.bufs + (long long)slot * 2 * a.max_frames * a.frame;
  const bool vec = a.vec && (wpos & 3) == 0;
  for (int f = wave; f < a.F; f += 4) {
    const int2 p = s_plan[f];
    if (p.x < 0) continue;
    const long long w0 = (long long)wpos + (long long)p.x * a.frame;  // r < F and F * frame <= ring_len: one wrap
    float* to = dst + (long long)p.y * a.frame;
    if (vec) {
      for (int k = 4 * lane; k < a.frame; k += 256) {
        const long long w = w0 + k;
        *reinterpret_cast<uint4*>(to + k) = *reinterpret_cast<const uint4*>(src + (w < a.ring_len ? w : w - a.ring_len));
      }
    } else {
      for (int k = lane; k < a.frame; k += 64) {
        const long long w = w0 + k;
        to[k] = src[w < a.ring_len ? w : w - a.ring_len];
      }
    }
  }
}

static bool host_aligned16(const void* p) { return ((unsigned long long)p & 15ull) == 0; }

const char* launch_turn(const float* staging, int S, int ring_len, const unsigned char* mask, const int* hdr, int A, int F,
                        int frame, int min_frames, int max_frames, float* bufs, int* state, int* totals, int* done,
                        hipStream_t s) {
  if (!staging || !mask || !hdr || !bufs || !state || !totals || !done) return "turn: null argument";
  if (A <= 0 || A > 65535) return "turn: 1 to 65535 rows";
  if (F < 1 || F > TURN_MAX_FRAMES) return "turn: 1 to 512 frames in a row";
  if (frame <= 0) return "turn: a frame is a positive number of samples";
  if (min_frames < F) return "turn: min_frames is at least the frames of a row (else a row could complete two turns)";
  if (min_frames > max_frames) return "turn: min_frames is at most max_frames";
  if (S <= 0 || (long long)F * frame > ring_len) return "turn: no slots, or a staging ring shorter than a row";
  if ((long long)max_frames * frame > 0x3fffffff) return "turn: a turn of more than 2^30 samples";
  TurnArgs a{staging, mask, hdr, bufs, state, totals, done, S, ring_len, F, frame, min_frames, max_frames,
             frame % 4 == 0 && ring_len % 4 == 0 && host_aligned16(staging) && host_aligned16(bufs)};
  hipLaunchKernelGGL(turn_kernel, dim3(A), dim3(256), 0, s, a);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

// out[r][k] = bufs[slot_r][buffer_r][k mod L_r], L_r = frames_r * frame, k < max_frames * frame: a turn tiled to the window
// (tile_crop_kernel's function with start 0).  rows (R, 3): slot, buffer, frames.  Grid (column tiles, R); four samples per
// lane where frame is a multiple of 4 and both bases are 16-byte aligned (L is then a multiple of 4: no 4-vector straddles
// the wrap), one sample per lane otherwise.  A row out of range writes nothing.
__global__ __launch_bounds__(256) void turn_collect_kernel(const float* __restrict__ bufs, int S, int max_frames, int frame,
                                                           const int* __restrict__ rows, float* __restrict__ out, int vec) {
  const int row = blockIdx.y, slot = rows[3 * row], buf = rows[3 * row + 1], frames = rows[3 * row + 2];
  if (slot < 0 || slot >= S || buf < 0 || buf > 1 || frames < 1 || frames > max_frames) return;
  const int W = max_frames * frame, L = frames * frame;
  const float* src = bufs + ((long long)slot * 2 + buf) * W;
  float* to = out + (long long)row * W;
  const int t = blockIdx.x * blockDim.x + threadIdx.x, step = gridDim.x * blockDim.x;
  if (vec) {
    for (int k = 4 * t; k < W; k += 4 * step)
      *reinterpret_cast<uint4*>(to + k) = *reinterpret_cast<const uint4*>(src + k % L);
  } else {
    for (int k = t; k < W; k += step) to[k] = src[k % L];
  }
}

const char* launch_turn_collect(const float* bufs, int S, int max_frames, int frame, const int* rows, int R, float* out,
                                hipStream_t s) {
  if (!bufs || !rows || !out) return "turn_collect: null argument";
  if (S <= 0 || R <= 0 || R > 65535) return "turn_collect: 1 to 65535 rows";
  if (frame <= 0 || max_frames <= 0 || (long long)max_frames * frame > 0x3fffffff)
    return "turn_collect: a window of 1 to 2^30 samples in whole frames";
  const int W = max_frames * frame, vec = frame % 4 == 0 && host_aligned16(bufs) && host_aligned16(out);
  const int per = vec ? 1024 : 256;
  hipLaunchKernelGGL(turn_collect_kernel, dim3(min((W + per - 1) / per, 64), R), dim3(256), 0, s, bufs, S, max_frames, frame,
                     rows, out, vec);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

// The close step of the recurrence (include/afx.h afx_k_turn_close): the end of a call.  One thread per named slot; a slot
// out of range, or whose state is no turn state, gets done = (-1, -1, -1, -1) and nothing else.
__global__ __launch_bounds__(256) void turn_close_kernel(const int* __restrict__ slots, int A, int S, int min_frames, int max_frames,
                                                         int* state, int* totals, int* __restrict__ done) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A) return;
  const int slot = slots[i];
  int open = 0, n = 0;
  bool ok = slot >= 0 && slot < S;
  if (ok) {
    open = state[3 * slot];
    n = state[3 * slot + 1];
    ok = (open == 0 || open == 1) && n >= 0 && n < max_frames;
  }
  int d0 = 0, d1 = 0, d2 = 0, d3 = 0;
  if (!ok) {
    d0 = d1 = d2 = d3 = -1;
  } else {
    if (n >= min_frames) {
      const int g = state[3 * slot + 2];
      d0 = open; d1 = n; d2 = g; d3 = g + n;
      totals[4 * slot] = turn_count(totals[4 * slot]);
      state[3 * slot] = open ^ 1;
    } else if (n > 0) {
      totals[4 * slot + 1] = turn_count(totals[4 * slot + 1]);
    }
    state[3 * slot + 1] = 0;
  }
  done[4 * i] = d0; done[4 * i + 1] = d1; done[4 * i + 2] = d2; done[4 * i + 3] = d3;
}

const char* launch_turn_close(const int* slots, int A, int S, int min_frames, int max_frames, int* state, int* totals, int* done,
                              hipStream_t s) {
  if (!slots || !state || !totals || !done) return "turn_close: null argument";
  if (A <= 0 || A > 65535) return "turn_close: 1 to 65535 rows";
  if (S <= 0) return "turn_close: no slots";
  if (min_frames < 1) return "turn_close: min_frames is at least 1";
  if (min_frames > max_frames) return "turn_close: min_frames is at most max_frames";
  hipLaunchKernelGGL(turn_close_kernel, dim3((A + 255) / 256), dim3(256), 0, s, slots, A, S, min_frames, max_frames, state, totals,
                     done);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

// ---------------------------------------------------------------------------------
// Turns offline (afx/turns.py score_turns; the functions are stated in include/afx.h afx_k_turn_scan / afx_k_turn_clips): the
// recurrence of turn_kernel over whole recordings at once.  The masks of A recordings stand back to back; one workgroup of 256
// threads per recording walks its mask TURN_SCAN_STEP frames a step, each thread one 16-byte load of 16 frames.  What makes
// the recurrence serial is only the state a thread's first frame meets, (n, g) of the open turn, and that follows from the
// start of the run the previous frame belongs to: a run of `run` frames before frame f0 leaves n = run % max_frames and
// g = f0 - n.  Per step:
//   load      16 mask bytes per thread, packed to 16 bits.  Chunks are aligned to 16 bytes of the ADDRESS, so a recording that
//             starts off that grid still loads 16 bytes a lane; only the chunks that hold a row's first or last frames (and the
//             one virtual not-kept frame behind the last that is the close step) go byte by byte;
//   starts    a frame starts a run when it is kept and the frame before it is not (the neighbour thread's last bit through
//             LDS, the last step's through the carry); the thread's last start, an exclusive max-scan over the workgroup
//             (__shfl_up within a wave, four wave totals through LDS) and the carry give the run start its first frame meets;
//   walk      the thread runs the stated recurrence over its 16 frames from that state and counts the turns it scores; an
//             exclusive sum-scan places them behind the turns of the step's earlier threads, of the earlier steps (the carry)
//             and of the earlier rows (row_base).  The table's order is the stream's: no atomic takes part in it.
// Three launches: the count pass (row counts into row_base, totals, open), one workgroup that turns the A counts into their
// exclusive prefix sums, and the write pass (the same walk, now storing).  Integer VALU, byte and 16-byte loads only.
// ---------------------------------------------------------------------------------
constexpr int TURN_SCAN_LANE = 16;                    // frames of a thread and step
constexpr int TURN_SCAN_STEP = 256 * TURN_SCAN_LANE;  // frames of a step (afx.turns.SCAN_STEP; include/afx.h states it)

struct TurnScanArgs {
  const unsigned char* mask;  // the rows' frames back to back: bit 0 = kept
  const long long* offs;      // (A + 1): row i is mask[offs[i] .. offs[i + 1])
  int* table;                 // (cap, 4): row, first, end, flags (bit 0 cut, bit 1 at_end)
  int* row_base;              // (A + 1): the count pass leaves row i's scored turns in [i]; then their exclusive prefix sums
  int* totals;                // (A, 4): scored, short, cut, kept
  int* open;                  // (A, 2): first, frames of the turn still open; (-1, 0): none
  int A, min_frames, max_frames, close_end, cap;
};

struct TurnScanMax { __device__ __forceinline__ int operator()(int a, int b) const { return max(a, b); } };
struct TurnScanSum { __device__ __forceinline__ int operator()(int a, int b) const { return a + b; } };

// An exclusive scan of v over the 256 threads in thread order, and its total: within a wave by __shfl_up, the four wave
// totals through s_wave.  Every thread of the workgroup calls it (two barriers).
template <class Op>
__device__ __forceinline__ int turn_scan_excl(int v, int ident, int* s_wave, Op op, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int u = __shfl_up(v, d, 64);
    if (lane >= d) v = op(u, v);
  }
  int mine = __shfl_up(v, 1, 64);
  if (lane == 0) mine = ident;
  __syncthreads();  // (the last scan's readers are done with s_wave)
  if (lane == 63) s_wave[wave] = v;
  __syncthreads();
  int before = ident;
  total = ident;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const int t = s_wave[w];
    if (w < wave) before = op(before, t);
    total = op(total, t);
  }
  return op(before, mine);
}

// The stated recurrence over the thread's frames f0 .. f0 + 15 (bit j of bits: frame f0 + j is kept), from (n, g); frames
// outside [0, end) are passed over, and frame n_row (there only with close_end: end = n_row + 1) is the close step.  -> the
// turns scored; with WRITE they go to table rows at, at + 1, ... below cap.
template <bool WRITE>
__device__ __forceinline__ int turn_scan_walk(unsigned bits, long long f0, long long end, int n_row, int n, int g, int min_frames,
                                              int max_frames, int& shrt, int& cut, int* table, long long at, int cap, int row) {
  int emitted = 0;
#pragma unroll
  for (int j = 0; j < TURN_SCAN_LANE; ++j) {
    const long long G = f0 + j;
    if (G < 0 || G >= end) continue;
    int first = -1, last = 0, flags = 0;
    if ((bits >> j) & 1) {
      if (n == 0) g = (int)G;
      if (++n == max_frames) {
        first = g; last = (int)G + 1; flags = 1;
        ++cut;
        n = 0;
      }
    } else if (n > 0) {
      if (n >= min_frames) {
        first = g; last = (int)G; flags = G == n_row ? 2 : 0;
      } else {
        ++shrt;
      }
      n = 0;
    }
    if (first >= 0) {
      if (WRITE && at + emitted < cap) {
        int* t = table + 4 * (at + emitted);
        t[0] = row; t[1] = first; t[2] = last; t[3] = flags;
      }
      ++emitted;
    }
  }
  return emitted;
}

template <bool WRITE>
__global__ __launch_bounds__(256) void turn_scan_kernel(TurnScanArgs a) {
  __shared__ int s_wave[4];
  __shared__ unsigned short s_bits[256];
  __shared__ int s_tot[3][4];
  const int row = blockIdx.x, tid = threadIdx.x;
  const long long o0 = a.offs[row], len = a.offs[row + 1] - o0;
  // (offsets that are negative, decrease or span 2^31 frames or more: the row is taken as one of no frames)
  const int n_row = o0 >= 0 && len > 0 && len < (1LL << 31) ? (int)len : 0;
  if (n_row == 0) {
    if (!WRITE && tid < 4) a.totals[4 * row + tid] = 0;
    if (!WRITE && tid < 2) a.open[2 * row + tid] = tid ? 0 : -1;
    if (!WRITE && tid == 0) a.row_base[row] = 0;
    return;
  }
  const unsigned char* m = a.mask + o0;
  const int mis = (int)((unsigned long long)m & 15ull);  // the row's first frame stands that far into a 16-byte group
  const long long end = (long long)n_row + (a.close_end ? 1 : 0);
  const long long at0 = WRITE ? a.row_base[row] : 0;
  int c_prev = 0, c_start = -1, c_scored = 0;  // the carry: was the step's last frame kept; the newest run start; turns scored
  int shrt = 0, cut = 0, kept = 0;             // this thread's share of the totals
  for (long long base = -mis; base < end; base += TURN_SCAN_STEP) {
    const long long f0 = base + tid * TURN_SCAN_LANE;
    unsigned bits = 0;
    if (f0 >= 0 && f0 + TURN_SCAN_LANE <= n_row) {
      const uint4 v = *reinterpret_cast<const uint4*>(m + f0);
      const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int k = 0; k < 4; ++k)
        bits |= ((w[k] & 1u) | ((w[k] >> 7) & 2u) | ((w[k] >> 14) & 4u) | ((w[k] >> 21) & 8u)) << (4 * k);
    } else {
#pragma unroll
      for (int j = 0; j < TURN_SCAN_LANE; ++j) {
        const long long f = f0 + j;
        if (f >= 0 && f < n_row) bits |= (unsigned)(m[f] & 1) << j;
      }
    }
    s_bits[tid] = (unsigned short)bits;
    __syncthreads();
    const int prev = tid ? (s_bits[tid - 1] >> 15) & 1 : c_prev;
    const int step_last = (s_bits[255] >> 15) & 1;
    const unsigned starts = bits & ~((bits << 1) | (unsigned)prev) & 0xffffu;
    const int my_start = starts ? (int)f0 + 31 - __clz(starts) : -1;
    int newest;
    const int before = max(c_start, turn_scan_excl(my_start, -1, s_wave, TurnScanMax(), newest));
    // the open turn this thread's first frame meets: the run it continues has f0 - before frames (1 to 2^31 - 1)
    const int n = prev ? (int)((unsigned)(f0 - before) % (unsigned)a.max_frames) : 0;
    const int g = (int)f0 - n;
    int d_short = 0, d_cut = 0, step_scored;
    const int mine = turn_scan_walk<false>(bits, f0, end, n_row, n, g, a.min_frames, a.max_frames, d_short, d_cut, nullptr, 0, 0, row);
    const int ahead = turn_scan_excl(mine, 0, s_wave, TurnScanSum(), step_scored);
    shrt += d_short; cut += d_cut; kept += __popc(bits);
    if (WRITE)
      turn_scan_walk<true>(bits, f0, end, n_row, n, g, a.min_frames, a.max_frames, d_short, d_cut, a.table,
                           at0 + c_scored + ahead, a.cap, row);
    c_prev = step_last;
    c_start = max(c_start, newest);
    c_scored += step_scored;
  }
  if (WRITE) return;
  // the totals: each wave sums its lanes, thread 0 the four waves
  int part[3] = {shrt, cut, kept};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) part[k] += __shfl_down(part[k], d, 64);
    if ((tid & 63) == 0) s_tot[k][tid >> 6] = part[k];
  }
  __syncthreads();
  if (tid == 0) {
    int* tot = a.totals + 4 * row;
    tot[0] = c_scored;
    for (int k = 0; k < 3; ++k) tot[1 + k] = s_tot[k][0] + s_tot[k][1] + s_tot[k][2] + s_tot[k][3];
    a.row_base[row] = c_scored;
    int first = -1, frames = 0;
    if (!a.close_end && (m[n_row - 1] & 1)) {  // the run at the row's end began at c_start; what a cut left of it is open
      frames = (int)((unsigned)(n_row - c_start) % (unsigned)a.max_frames);
      first = frames ? n_row - frames : -1;
    }
    a.open[2 * row] = first;
    a.open[2 * row + 1] = frames;
  }
}

// row_base[i] <- the sum of row_base[0 .. i), i = 0 .. A, clamped to 2^31 - 1: one workgroup, a contiguous share per thread
__global__ __launch_bounds__(256) void turn_scan_base_kernel(int* row_base, int A) {
  __shared__ long long s_sum[256];
  const int tid = threadIdx.x, per = (A + 255) / 256, lo = min(tid * per, A), hi = min(lo + per, A);
  long long sum = 0;
  for (int i = lo; i < hi; ++i) sum += row_base[i];
  s_sum[tid] = sum;
  __syncthreads();
  long long run = 0;
  for (int t = 0; t < tid; ++t) run += s_sum[t];
  for (int i = lo; i < hi; ++i) {
    const int c = row_base[i];
    row_base[i] = (int)min(run, 0x7fffffffLL);
    run += c;
  }
  if (tid == 255) row_base[A] = (int)min(run, 0x7fffffffLL);  // (the shares end at A: behind the last one `run` is the total)
}

const char* launch_turn_scan(const unsigned char* mask, const long long* offs, int A, int min_frames, int max_frames,
                             int close_end, int* table, int cap, int* row_base, int* totals, int* open, hipStream_t s) {
  if (!mask || !offs || !table || !row_base || !totals || !open) return "turn_scan: null argument";
  if (A <= 0 || A > 65535) return "turn_scan: 1 to 65535 rows";
  if (min_frames < 1) return "turn_scan: min_frames is at least 1";
  if (min_frames > max_frames) return "turn_scan: min_frames is at most max_frames";
  if (cap < 0) return "turn_scan: a table of 0 or more rows";
  TurnScanArgs a{mask, offs, table, row_base, totals, open, A, min_frames, max_frames, close_end ? 1 : 0, cap};
  hipLaunchKernelGGL(turn_scan_kernel<false>, dim3(A), dim3(256), 0, s, a);
  hipLaunchKernelGGL(turn_scan_base_kernel, dim3(1), dim3(256), 0, s, row_base, A);
  if (cap > 0) hipLaunchKernelGGL(turn_scan_kernel<true>, dim3(A), dim3(256), 0, s, a);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

// out[r][k] = x[xoffs[row] + first * frame + k mod L], L = (end - first) * frame, k < max_frames * frame, (row, first, end)
// from table row r, read on the device: a scored turn is contiguous in its recording, so its clip is tiled from the source
// (turn_collect_kernel's function without the buffers).  Grid (column tiles, R); four samples per lane where frame is a
// multiple of 4, out is 16-byte aligned and the turn's first sample is; one sample per lane otherwise.  A row that names no
// turn of its recording writes nothing.
__global__ __launch_bounds__(256) void turn_clips_kernel(const float* __restrict__ x, const long long* __restrict__ xoffs, int A,
                                                         int frame, int max_frames, const int* __restrict__ table,
                                                         float* __restrict__ out, int vec) {
  const int r = blockIdx.y;
  const int* t = table + 4 * (long long)r;
  const int row = t[0], first = t[1], end = t[2];
  if (row < 0 || row >= A || first < 0 || end <= first || end - first > max_frames) return;
  const long long x0 = xoffs[row], x1 = xoffs[row + 1];
  if (x0 < 0 || (long long)end * frame > x1 - x0) return;
  const int W = max_frames * frame, L = (end - first) * frame;
  const float* src = x + x0 + (long long)first * frame;
  float* to = out + (long long)r * W;
  const int i = blockIdx.x * blockDim.x + threadIdx.x, step = gridDim.x * blockDim.x;
  if (vec && ((unsigned long long)src & 15ull) == 0) {
    for (int k = 4 * i; k < W; k += 4 * step)
      *reinterpret_cast<uint4*>(to + k) = *reinterpret_cast<const uint4*>(src + k % L);
  } else {
    for (int k = i; k < W; k += step) to[k] = src[k % L];
  }
}

const char* launch_turn_clips(const float* x, const long long* xoffs, int A, int frame, int max_frames, const int* table, int r0,
                              int R, float* out, hipStream_t s) {
  if (!x || !xoffs || !table || !out) return "turn_clips: null argument";
  if (A <= 0) return "turn_clips: no recordings";
  if (r0 < 0 || R <= 0 || R > 65535) return "turn_clips: 1 to 65535 table rows from row r0 >= 0";
  if (frame <= 0 || max_frames <= 0 || (long long)max_frames * frame > 0x3fffffff)
    return "turn_clips: a window of 1 to 2^30 samples in whole frames";
  const int W = max_frames * frame, vec = frame % 4 == 0 && host_aligned16(out);
  const int per = vec ? 1024 : 256;
  hipLaunchKernelGGL(turn_clips_kernel, dim3(min((W + per - 1) / per, 64), R), dim3(256), 0, s, x, xoffs, A, frame, max_frames,
                     table + 4 * (long long)r0, out, vec);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

// ---------------------------------------------------------------------------------
// Cascade (afx/cascade.py; the functions are stated in include/afx.h afx_k_cascade_store / _select / _windows): a cheap
// screen scores every slot at every hop, and the windows of the slots whose score looks suspicious are gathered for a
// second model.  Three launches per push, every index from a host-built header:
//   store:   the hop of each named slot into its row of the retained-audio ring hist (S, window), sample t of a session
//            at column t mod window (the layout of SlidingWindowScorer.ring);
//   select:  ONE workgroup ranks the candidates (eligible, not cooling down, score < threshold) by (score, slot), writes
//            the `budget` first row positions to sel and advances every named slot's cooldown counter;
//   windows: reads sel from device memory and gathers the chosen slots' windows, oldest sample first, tiled while the
//            session is younger than the window (afx_k_tile_crop's function), into a dense batch.
// ---------------------------------------------------------------------------------
constexpr int CASCADE_MAX_ROWS = 8192;     // rows of one select launch: 8-byte keys in 64 KB of LDS (include/afx.h states it)
constexpr int CASCADE_SELECT_THREADS = 1024;
constexpr int CASCADE_PER_THREAD = CASCADE_MAX_ROWS / CASCADE_SELECT_THREADS;

__device__ __forceinline__ bool aligned16(const void* p) { return ((unsigned long long)p & 15ull) == 0; }

// hist[slot_i][(wpos_i + k) mod window] = x[i][k], k < hop.  hdr (A, 2): slot, wpos.  Four samples per lane where the row's
// source and destination are 16-byte aligned and no group of four straddles the wrap (wpos, hop and window multiples of
// 4); one sample per lane otherwise.
__global__ __launch_bounds__(256) void cascade_store_kernel(const float* __restrict__ x, const int* __restrict__ hdr,
                                                            float* __restrict__ hist, int S, int window, int hop) {
  const int row = blockIdx.y, slot = hdr[2 * row], wpos = hdr[2 * row + 1];
  if (!(slot >= 0 && slot < S && wpos >= 0 && wpos < window)) return;
  const float* src = x + (long long)row * hop;
  float* dst = hist + (long long)slot * window;
  const int t0 = blockIdx.x * blockDim.x + threadIdx.x, step = gridDim.x * blockDim.x;
  if (((wpos | hop | window) & 3) == 0 && aligned16(src) && aligned16(dst)) {
    for (int q = t0; q < hop / 4; q += step) {
      const int w = wpos + 4 * q;
      *reinterpret_cast<float4*>(dst + (w < window ? w : w - window)) = *reinterpret_cast<const float4*>(src + 4 * q);
    }
    return;
  }
  for (int k = t0; k < hop; k += step) {
    const int w = wpos + k;  // hop <= window: one wrap
    dst[w < window ? w : w - window] = src[k];
  }
}

const char* launch_cascade_store(const float* x, int A, int hop, const int* hdr, float* hist, int S, int window,
                                 hipStream_t s) {
  if (!x || !hdr || !hist) return "cascade_store: null argument";
  if (A <= 0 || A > 65535) return "cascade_store: 1 to 65535 rows";
  if (S <= 0 || window <= 0 || hop <= 0 || hop > window) return "cascade_store: a hop must be positive and fit the window";
  hipLaunchKernelGGL(cascade_store_kernel, dim3(min((hop + 1023) / 1024, 64), A), dim3(256), 0, s, x, hdr, hist, S, window, hop);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

// (score, slot) -> a 64-bit key whose unsigned order is before(): scores ascending with -0.0 and +0.0 equal, then the lower
// slot.  Never called for a NaN (a NaN is no candidate).  The slots of a launch are distinct, so the keys are too.
__device__ __forceinline__ unsigned long long cascade_key(float score, int slot) {
  unsigned int u = __float_as_uint(score);
  if (u == 0x80000000u) u = 0u;                              // -0.0 ties with +0.0
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);            // monotone: -inf lowest, +inf highest
  return ((unsigned long long)u << 32) | (unsigned int)slot;
}

// One workgroup of 16 waves; thread t owns rows t, t + 1024, ... (at most CASCADE_PER_THREAD) and keeps their keys in
// registers.  Candidates are compacted into LDS (wave ballot + popcount prefix, wave bases from a 16-entry table that the
// keys then overwrite), then each owner counts the keys below its own: that count is the rank, all keys being distinct.
__global__ __launch_bounds__(CASCADE_SELECT_THREADS) void cascade_select_kernel(const float* __restrict__ scores, int stride,
                                                                                const int* __restrict__ hdr, int A,
                                                                                int* __restrict__ wait, int* __restrict__ counts,
                                                                                int S, float threshold, int budget, int cooldown,
                                                                                int* __restrict__ sel) {
  extern __shared__ __attribute__((aligned(16))) unsigned char cascade_lds[];
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(cascade_lds);
  int* wave_total = reinterpret_cast<int*>(cascade_lds);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const unsigned long long below = (1ull << lane) - 1ull;
  unsigned long long key[CASCADE_PER_THREAD];
  int w_old[CASCADE_PER_THREAD];
  unsigned int named = 0, cand = 0;  // bit k: row tid + 1024 k has a slot inside the state / is a candidate
  int mine = 0;                      // candidates of this wave
#pragma unroll
  for (int k = 0; k < CASCADE_PER_THREAD; ++k) {
    const int i = tid + k * CASCADE_SELECT_THREADS;
    bool c = false;
    key[k] = 0ull;
    w_old[k] = 0;
    if (i < A) {
      const int slot = hdr[2 * i];
      if (slot >= 0 && slot < S) {
        named |= 1u << k;
        const float sc = scores[(long long)i * stride];
        w_old[k] = wait[slot];
        c = hdr[2 * i + 1] != 0 && w_old[k] == 0 && sc < threshold;  // (false for a NaN score)
        if (c) {
          cand |= 1u << k;
          key[k] = cascade_key(sc, slot);
        }
      }
    }
    mine += __popcll(__ballot(c));
  }
  if (lane == 0) wave_total[wave] = mine;
  __syncthreads();
  int base = 0, total = 0;
#pragma unroll
  for (int w = 0; w < CASCADE_SELECT_THREADS / 64; ++w) {
    const int t = wave_total[w];
    base += w < wave ? t : 0;
    total += t;
  }
  __syncthreads();  // every wave has read the table: the keys may take its place
#pragma unroll
  for (int k = 0; k < CASCADE_PER_THREAD; ++k) {
    const bool c = (cand >> k) & 1u;
    const unsigned long long b = __ballot(c);
    if (c) keys[base + __popcll(b & below)] = key[k];
    base += __popcll(b);
  }
  __syncthreads();
  if (tid == 0) sel[0] = min(total, budget);
  int rank[CASCADE_PER_THREAD];
#pragma unroll
  for (int k = 0; k < CASCADE_PER_THREAD; ++k) rank[k] = 0;
  if (cand) {
    for (int c = 0; c < total; ++c) {
      const unsigned long long o = keys[c];  // one address for the whole wave: a broadcast read
#pragma unroll
      for (int k = 0; k < CASCADE_PER_THREAD; ++k) rank[k] += o < key[k] ? 1 : 0;
    }
  }
#pragma unroll
  for (int k = 0; k < CASCADE_PER_THREAD; ++k) {
    if (!((named >> k) & 1u)) continue;
    const int i = tid + k * CASCADE_SELECT_THREADS;
    const bool chosen = ((cand >> k) & 1u) && rank[k] < budget;
    const int slot = hdr[2 * i];
    if (chosen) sel[1 + rank[k]] = i;
    wait[slot] = chosen ? cooldown : max(w_old[k] - 1, 0);
    if (counts && ((cand >> k) & 1u)) {  // (the slot is this thread's alone: plain adds)
      counts[2 * slot] += 1;
      counts[2 * slot + 1] += chosen ? 0 : 1;
    }
  }
}

const char* launch_cascade_select(const float* scores, int stride, const int* hdr, int A, int* wait, int* counts, int S,
                                  float threshold, int budget, int cooldown, int* sel, hipStream_t s) {
  if (!scores || !hdr || !wait || !sel) return "cascade_select: null argument";
  if (stride < 1) return "cascade_select: a score stride of at least 1";
  if (A <= 0 || A > CASCADE_MAX_ROWS) return "cascade_select: 1 to 8192 rows";
  if (S <= 0) return "cascade_select: no slots";
  if (threshold != threshold) return "cascade_select: the threshold is NaN";
  if (budget < 1 || cooldown < 0) return "cascade_select: budget >= 1 and cooldown >= 0";
  const size_t lds = (size_t)max(A, 16) * sizeof(unsigned long long);
  hipLaunchKernelGGL(cascade_select_kernel, dim3(1), dim3(CASCADE_SELECT_THREADS), lds, s, scores, stride, hdr, A, wait, counts,
                     S, threshold, budget, cooldown, sel);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

// out[r][j] = hist[slot_i][(start_i + j) mod n_i], j < window, for r < sel[0] and i = sel[1 + r].  hdr (A, 3): slot, n,
// start.  A steady row (n = window) copies four samples per lane where start and window are multiples of 4 and both rows
// 16-byte aligned; a warm row (n < window, the history tiled) and every other steady row take one sample per lane.
__global__ __launch_bounds__(256) void cascade_windows_kernel(const float* __restrict__ hist, int S, int window,
                                                              const int* __restrict__ hdr, int A, const int* __restrict__ sel,
                                                              int budget, float* __restrict__ out) {
  const int r = blockIdx.y;
  if (r >= min(sel[0], budget)) return;
  const int i = sel[1 + r];
  if (i < 0 || i >= A) return;
  const int slot = hdr[3 * i], n = hdr[3 * i + 1], start = hdr[3 * i + 2];
  if (!(slot >= 0 && slot < S && n >= 1 && n <= window && start >= 0 && start < n)) return;
  const float* src = hist + (long long)slot * window;
  float* dst = out + (long long)r * window;
  const int t0 = blockIdx.x * blockDim.x + threadIdx.x, step = gridDim.x * blockDim.x;
  if (n == window) {
    if (((start | window) & 3) == 0 && aligned16(src) && aligned16(dst)) {
      for (int q = t0; q < window / 4; q += step) {
        const int c = start + 4 * q;
        *reinterpret_cast<float4*>(dst + 4 * q) = *reinterpret_cast<const float4*>(src + (c < window ? c : c - window));
      }
      return;
    }
    for (int j = t0; j < window; j += step) {
      const int c = start + j;
      dst[j] = src[c < window ? c : c - window];
    }
    return;
  }
  for (int j = t0; j < window; j += step) dst[j] = src[(int)(((long long)start + j) % n)];
}

const char* launch_cascade_windows(const float* hist, int S, int window, const int* hdr, int A, const int* sel, int budget,
                                   float* out, hipStream_t s) {
  if (!hist || !hdr || !sel || !out) return "cascade_windows: null argument";
  if (S <= 0 || window <= 0 || A <= 0) return "cascade_windows: no slots, no window or no rows";
  if (budget < 1 || budget > 65535) return "cascade_windows: a budget of 1 to 65535 rows";
  hipLaunchKernelGGL(cascade_windows_kernel, dim3(min((window + 1023) / 1024, 64), budget), dim3(256), 0, s, hist, S, window,
                     hdr, A, sel, budget, out);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

// ---------------------------------------------------------------------------------
// Verdicts (afx/verdict.py; the function is stated in include/afx.h afx_k_verdict): per-slot smoothing, hysteresis and an
// event log over the scores of one push.  ONE workgroup of 16 waves takes the rows in chunks of 1024, in row order; thread t
// of a chunk runs its row's state machine (the slots of a launch are distinct: the state row is the thread's alone).  The
// events of a chunk get their log positions from a wave ballot + popcount prefix, the 16 wave totals are prefixed through
// LDS onto a running base that starts at log[0]: ascending row position within a launch, launches in stream order, no
// atomics.  Events at or past cap are counted, not stored.
// ---------------------------------------------------------------------------------
constexpr int VERDICT_MAX_ROWS = 8192;
constexpr int VERDICT_THREADS = 1024;
constexpr int VERDICT_N_MAX = 0x7fffffff;

__global__ __launch_bounds__(VERDICT_THREADS) void verdict_kernel(const float* __restrict__ scores, int stride,
                                                                  const float* __restrict__ vscores, const int* __restrict__ hdr,
                                                                  int A, float* __restrict__ m, int* __restrict__ st, int S,
                                                                  float alpha, float enter, float exit_, float verifier_enter,
                                                                  int confirm, int release, int min_scores, int latch,
                                                                  int* __restrict__ log, int cap) {
  __shared__ int wave_total[VERDICT_THREADS / 64];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const unsigned long long below = (1ull << lane) - 1ull;
  long long base = log[0];  // (every thread reads it before the first barrier; thread 0 stores the new count after the last)
  for (int row0 = 0; row0 < A; row0 += VERDICT_THREADS) {
    const int i = row0 + tid;
    int kind = 0, slot = -1, k = 0;
    float m1 = 0.f;
    if (i < A) {
      slot = hdr[2 * i];
      k = hdr[2 * i + 1];
      const float s = scores[(long long)i * stride];
      if (slot >= 0 && slot < S && !(s != s)) {  // a NaN score: "no hop completed", the row changes nothing
#pragma clang fp contract(off)
        const float v = vscores ? vscores[i] : __builtin_nanf("");
        const bool has_v = !(v != v);
        int* q = st + 4ll * slot;
        const int n = q[0];
        int run = q[1], on = q[2], since = q[3];
        const int n1 = n == VERDICT_N_MAX ? n : n + 1;
        if (n == 0) {
          m1 = s;
        } else {
          const float mo = m[slot];
          const float d = s - mo;
          const float p = alpha * d;
          m1 = mo + p;
        }
        if (on == 0) {
          if (has_v && v < verifier_enter) {
            on = 1, run = 0, since = k, kind = 2;
          } else if (has_v) {
            run = 0;
          } else if (n1 >= min_scores && m1 < enter) {
            run += 1;
            if (run >= confirm) on = 1, run = 0, since = k, kind = 1;
          } else {
            run = 0;
          }
        } else if (!latch) {
          if (m1 >= exit_) {
            run += 1;
            if (run >= release) on = 0, run = 0, since = -1, kind = 3;
          } else {
            run = 0;
          }
        }
        m[slot] = m1;
        q[0] = n1, q[1] = run, q[2] = on, q[3] = since;
      }
    }
    const unsigned long long b = __ballot(kind != 0);
    if (lane == 0) wave_total[wave] = __popcll(b);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < VERDICT_THREADS / 64; ++w) {
      const int t = wave_total[w];
      before += w < wave ? t : 0;
      total += t;
    }
    if (kind != 0) {
      const long long e = base + before + __popcll(b & below);
      if (e >= 0 && e < cap) {
        int* dst = log + 1 + 4 * e;
        dst[0] = slot, dst[1] = kind, dst[2] = k, dst[3] = __float_as_int(m1);
      }
    }
    base += total;
    __syncthreads();  // every wave has read the table: the next chunk may overwrite it
  }
  if (tid == 0) log[0] = (int)min(base, (long long)VERDICT_N_MAX);
}

const char* launch_verdict(const float* scores, int stride, const float* vscores, const int* hdr, int A, float* m, int* st,
                           int S, float alpha, float enter, float exit_, float verifier_enter, int confirm, int release,
                           int min_scores, int latch, int* log, int cap, hipStream_t s) {
  if (!scores || !hdr || !m || !st || !log) return "verdict: null argument";
  if (stride < 1) return "verdict: a score stride of at least 1";
  if (A <= 0 || A > VERDICT_MAX_ROWS) return "verdict: 1 to 8192 rows";
  if (S <= 0) return "verdict: no slots";
  if (!(alpha > 0.f && alpha <= 1.f)) return "verdict: alpha in (0, 1]";
  if (enter != enter || exit_ != exit_) return "verdict: a threshold is NaN";
  if (verifier_enter != verifier_enter) return "verdict: the verifier threshold is NaN";
  if (exit_ < enter) return "verdict: exit below enter";
  if (confirm < 1 || release < 1 || min_scores < 1) return "verdict: confirm, release and min_scores of at least 1";
  if (latch != 0 && latch != 1) return "verdict: latch is 0 or 1";
  if (cap < 0) return "verdict: a negative log capacity";
  hipLaunchKernelGGL(verdict_kernel, dim3(1), dim3(VERDICT_THREADS), 0, s, scores, stride, vscores, hdr, A, m, st, S, alpha, enter,
                     exit_, verifier_enter, confirm, release, min_scores, latch, log, cap);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

// ---------------------------------------------------------------------------------
// Evidence clips (afx/evidence.py; the function is stated in include/afx.h afx_k_evidence_mark / _copy): a pre-roll ring of
// audio and scores per slot, and a pool of clips that an alarm raised by this push fills with the pre-roll, the raising hop
// and a post-roll.  Two launches per update, every index from a host-built header and the verdict state on the device:
//   mark:  ONE workgroup of 16 waves.  It lists the free pool entries in ascending index (ballot + popcount prefix into
//          LDS), settles which row owns a slot named twice (the lowest row position, through an atomic min on a scratch
//          word per slot), then takes the rows in chunks of 1024 in row order: a recording slot appends, a raising slot
//          takes the free entry of its rank among the raising rows.  It updates rec, left, the clip headers and the four
//          counters and leaves one work item per row;
//   copy:  a grid over rows x hop tiles carries the work items out: the hop into the ring, into its clip, and for an
//          opened clip the pre-roll out of the ring, fp32 bit for bit or as pcm16.
// ---------------------------------------------------------------------------------
constexpr int EVIDENCE_MAX_ROWS = 8192;
constexpr int EVIDENCE_MAX_CLIPS = 8192;  // the free list: 32 KB of LDS (include/afx.h states it)
constexpr int EVIDENCE_THREADS = 1024;
constexpr int EVIDENCE_FREE = 0, EVIDENCE_RECORDING = 1, EVIDENCE_COMPLETE = 2;
constexpr int EVIDENCE_UNCLAIMED = 0x7fffffff;

__global__ __launch_bounds__(EVIDENCE_THREADS) void evidence_mark_kernel(const int* __restrict__ hdr, int A,
                                                                         const int* __restrict__ vst, int S, int pre, int post,
                                                                         int* __restrict__ rec, int* __restrict__ left, int* claim,
                                                                         int* __restrict__ pool, int clips,
                                                                         int* __restrict__ counters, int* __restrict__ work) {
  __shared__ int s_free[EVIDENCE_MAX_CLIPS];
  __shared__ int wave_total[EVIDENCE_THREADS / 64];
  __shared__ int s_merged;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const unsigned long long below = (1ull << lane) - 1ull;
  const int recorded0 = counters[1];  // (every thread reads it before the first barrier; thread 0 stores after the last)
  const int L = pre + 1 + post;
  if (tid == 0) s_merged = 0;
  // the free entries in ascending index
  int nfree = 0;
  for (int e0 = 0; e0 < clips; e0 += EVIDENCE_THREADS) {
    const int e = e0 + tid;
    const bool fr = e < clips && pool[6 * e] == EVIDENCE_FREE;
    const unsigned long long b = __ballot(fr);
    if (lane == 0) wave_total[wave] = __popcll(b);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < EVIDENCE_THREADS / 64; ++w) {
      const int t = wave_total[w];
      before += w < wave ? t : 0;
      total += t;
    }
    if (fr) s_free[nfree + before + __popcll(b & below)] = e;
    nfree += total;
    __syncthreads();
  }
  // a slot named twice belongs to the lowest row position that names it
  for (int i = tid; i < A; i += EVIDENCE_THREADS) {
    const int slot = hdr[2 * i], k = hdr[2 * i + 1];
    if (slot >= 0 && slot < S && k >= 1) atomicMin(&claim[slot], i);
  }
  __threadfence();  // the claims have reached memory before any wave reads one
  __syncthreads();
  int base = 0;  // raising rows before this chunk
  for (int row0 = 0; row0 < A; row0 += EVIDENCE_THREADS) {
    const int i = row0 + tid;
    int op = -1, entry = 0, wa = 0, wb = 0, slot = -1, k = 0;
    bool opens = false, merges = false;
    if (i < A) {
      slot = hdr[2 * i];
      k = hdr[2 * i + 1];
      if (slot >= 0 && slot < S && k >= 1 && __hip_atomic_load(&claim[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == i) {
        const bool raise = vst[4ll * slot + 2] == 1 && vst[4ll * slot + 3] == k;
        const int r = rec[slot];
        op = 0;
        if (r >= 0 && r < clips && pool[6 * r + 4] < L) {  // recording: the hop is appended
          int* h = pool + 6 * r;
          merges = raise;
          op = 1, entry = r, wa = h[4];
          h[4] = wa + 1;
          const int l = left[slot] - 1;
          if (l <= 0) h[0] = EVIDENCE_COMPLETE, rec[slot] = -1;
          left[slot] = max(l, 0);
        } else {
          opens = raise;
        }
      }
    }
    const unsigned long long bm = __ballot(merges);
    if (lane == 0 && bm) atomicAdd(&s_merged, __popcll(bm));
    const unsigned long long b = __ballot(opens);
    if (lane == 0) wave_total[wave] = __popcll(b);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < EVIDENCE_THREADS / 64; ++w) {
      const int t = wave_total[w];
      before += w < wave ? t : 0;
      total += t;
    }
    if (opens) {
      const int rank = base + before + __popcll(b & below);
      if (rank < nfree) {  // else dropped: the hop is stored in the ring and nothing more
        const int e = s_free[rank], f = max(1, k - pre);
        int* h = pool + 6 * e;
        h[0] = post == 0 ? EVIDENCE_COMPLETE : EVIDENCE_RECORDING;
        h[1] = slot, h[2] = k, h[3] = f, h[4] = k - f + 1, h[5] = recorded0 + rank;
        if (post > 0) rec[slot] = e, left[slot] = post;
        op = 2, entry = e, wa = f, wb = k - f + 1;
      }
    }
    if (i < A) {
      int* w = work + 4ll * i;
      w[0] = op, w[1] = entry, w[2] = wa, w[3] = wb;
    }
    base += total;
    __syncthreads();  // every wave has read the table: the next chunk may overwrite it
  }
  // the scratch words go back to "unclaimed" for the next launch (every claim was read before the last barrier)
  for (int i = tid; i < A; i += EVIDENCE_THREADS) {
    const int slot = hdr[2 * i], k = hdr[2 * i + 1];
    if (slot >= 0 && slot < S && k >= 1) __hip_atomic_store(&claim[slot], EVIDENCE_UNCLAIMED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (tid == 0) {
    const int got = min(base, nfree);
    counters[0] += base;
    counters[1] = recorded0 + got;
    counters[2] += base - got;
    counters[3] += s_merged;
  }
}

const char* launch_evidence_mark(const int* hdr, int A, const int* vst, int S, int pre, int post, int* rec, int* left, int* claim,
                                 int* pool, int clips, int* counters, int* work, hipStream_t s) {
  if (!hdr || !vst || !rec || !left || !claim || !pool || !counters || !work) return "evidence_mark: null argument";
  if (A <= 0 || A > EVIDENCE_MAX_ROWS) return "evidence_mark: 1 to 8192 rows";
  if (S <= 0) return "evidence_mark: no slots";
  if (pre < 0 || post < 0 || (long long)pre + post + 1 > 0x7fffffffll) return "evidence_mark: pre and post of 0 or more hops";
  if (clips < 1 || clips > EVIDENCE_MAX_CLIPS) return "evidence_mark: 1 to 8192 clips";
  hipLaunchKernelGGL(evidence_mark_kernel, dim3(1), dim3(EVIDENCE_THREADS), 0, s, hdr, A, vst, S, pre, post, rec, left, claim, pool,
                     clips, counters, work);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

// q = x * 32768 (one fp32 multiply), NaN -> 0, clamped to [-32768, 32767], rounded half to even
__device__ __forceinline__ short evidence_pcm16(float x) {
  float q = x * 32768.f;
  q = (q != q) ? 0.f : q;
  q = fminf(fmaxf(q, -32768.f), 32767.f);
  return (short)(int)__builtin_rintf(q);
}

// one hop from src to dst_f (fp32, bit for bit) or dst_h (pcm16): four samples per lane where the hop is a multiple of 4
// and both rows are aligned for it (16 bytes of fp32, 8 of int16), one sample per lane otherwise
__device__ __forceinline__ void evidence_put(const float* __restrict__ src, float* __restrict__ dst_f, short* __restrict__ dst_h,
                                             int hop, int t0, int step) {
  if (dst_f) {
    if ((hop & 3) == 0 && aligned16(src) && aligned16(dst_f)) {
      for (int q = t0; q < hop / 4; q += step)
        *reinterpret_cast<uint4*>(dst_f + 4 * q) = *reinterpret_cast<const uint4*>(src + 4 * q);
      return;
    }
    const unsigned int* s = reinterpret_cast<const unsigned int*>(src);
    unsigned int* d = reinterpret_cast<unsigned int*>(dst_f);
    for (int j = t0; j < hop; j += step) d[j] = s[j];
    return;
  }
  if ((hop & 3) == 0 && aligned16(src) && ((unsigned long long)dst_h & 7ull) == 0) {
    for (int q = t0; q < hop / 4; q += step) {
      const float4 v = *reinterpret_cast<const float4*>(src + 4 * q);
      short4 o;
      o.x = evidence_pcm16(v.x), o.y = evidence_pcm16(v.y), o.z = evidence_pcm16(v.z), o.w = evidence_pcm16(v.w);
      *reinterpret_cast<short4*>(dst_h + 4 * q) = o;
    }
    return;
  }
  for (int j = t0; j < hop; j += step) dst_h[j] = evidence_pcm16(src[j]);
}

struct EvidenceCopyArgs {
  const float* x;       // (A, hop) the hops of this update
  const float* scores;  // score of row i at scores[i * stride], or nullptr: every score is NaN
  const int* hdr;       // (A, 2): slot, k
  const int* work;      // (A, 4): what evidence_mark left
  float* hist;          // (S, (pre + 1) hop)
  float* sring;         // (S, pre + 1)
  void* audio;          // (clips, L hop) fp32 or int16
  float* cscores;       // (clips, L)
  int stride, A, hop, pre, post, S, clips, pcm16;
};

__global__ __launch_bounds__(256) void evidence_copy_kernel(EvidenceCopyArgs a) {
  const int row = blockIdx.y;
  const int slot = a.hdr[2 * row], k = a.hdr[2 * row + 1];
  const int op = a.work[4 * row], entry = a.work[4 * row + 1], wa = a.work[4 * row + 2], wb = a.work[4 * row + 3];
  const int P = a.pre + 1, L = P + a.post;
  if (!(slot >= 0 && slot < a.S && k >= 1 && op >= 0 && op <= 2)) return;
  if (op == 1 && !(entry >= 0 && entry < a.clips && wa >= 0 && wa < L)) return;
  if (op == 2 && !(entry >= 0 && entry < a.clips && wa >= 1 && wb >= 1 && wb <= P && wa + (wb - 1) == k)) return;
  const int t0 = blockIdx.x * blockDim.x + threadIdx.x, step = gridDim.x * blockDim.x;
  const int c = (k - 1) % P;
  const float* src = a.x + (long long)row * a.hop;
  float* ring = a.hist + (long long)slot * P * a.hop;
  evidence_put(src, ring + (long long)c * a.hop, nullptr, a.hop, t0, step);
  const long long clip0 = (long long)entry * L * a.hop;
  float* clip_f = a.pcm16 ? nullptr : static_cast<float*>(a.audio) + clip0;
  short* clip_h = a.pcm16 ? static_cast<short*>(a.audio) + clip0 : nullptr;
  if (op >= 1) {  // this hop, from the update's own rows: position wa of a clip being recorded, the last of an opened one
    const long long at = (long long)(op == 1 ? wa : wb - 1) * a.hop;
    evidence_put(src, clip_f ? clip_f + at : nullptr, clip_h ? clip_h + at : nullptr, a.hop, t0, step);
  }
  if (op == 2) {  // the pre-roll: hops wa .. k - 1 out of the ring (none of them is written by this launch)
    for (int j = 0; j < wb - 1; ++j) {
      const float* from = ring + (long long)((wa - 1 + j) % P) * a.hop;
      const long long at = (long long)j * a.hop;
      evidence_put(from, clip_f ? clip_f + at : nullptr, clip_h ? clip_h + at : nullptr, a.hop, t0, step);
    }
  }
  if (blockIdx.x == 0) {  // the scores beside the audio
    const float s = a.scores ? a.scores[(long long)row * a.stride] : __builtin_nanf("");
    float* sr = a.sring + (long long)slot * P;
    float* cs = a.cscores + (long long)entry * L;
    if (threadIdx.x == 0) {
      sr[c] = s;
      if (op == 1) cs[wa] = s;
      if (op == 2) cs[wb - 1] = s;
    }
    if (op == 2)
      for (int j = threadIdx.x; j < wb - 1; j += blockDim.x) cs[j] = sr[(wa - 1 + j) % P];
  }
}

const char* launch_evidence_copy(const float* x, const float* scores, int stride, const int* hdr, const int* work, int A, int hop,
                                 int pre, int post, float* hist, float* sring, int S, void* audio, float* cscores, int clips,
                                 int encoding, hipStream_t s) {
  if (!x || !hdr || !work || !hist || !sring || !audio || !cscores) return "evidence_copy: null argument";
  if (scores && stride < 1) return "evidence_copy: a score stride of at least 1";
  if (A <= 0 || A > EVIDENCE_MAX_ROWS) return "evidence_copy: 1 to 8192 rows";
  if (S <= 0 || hop <= 0) return "evidence_copy: no slots or no hop";
  if (pre < 0 || post < 0 || ((long long)pre + 1) * hop > 0x7fffffffll || ((long long)pre + 1 + post) * hop > 0x7fffffffll)
    return "evidence_copy: pre and post of 0 or more hops, a ring and a clip below 2^31 samples";
  if (clips < 1 || clips > EVIDENCE_MAX_CLIPS) return "evidence_copy: 1 to 8192 clips";
  if (encoding != 0 && encoding != 1) return "evidence_copy: encoding 0 (fp32) or 1 (pcm16)";
  EvidenceCopyArgs a{};
  a.x = x; a.scores = scores; a.hdr = hdr; a.work = work; a.hist = hist; a.sring = sring; a.audio = audio; a.cscores = cscores;
  a.stride = scores ? stride : 0; a.A = A; a.hop = hop; a.pre = pre; a.post = post; a.S = S; a.clips = clips; a.pcm16 = encoding;
  hipLaunchKernelGGL(evidence_copy_kernel, dim3(min((hop + 1023) / 1024, 64), A), dim3(256), 0, s, a);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

// ---------------------------------------------------------------------------------
// Input quality (afx/quality.py; the function is stated in include/afx.h afx_k_quality): what the hop behind each score
// looked like -- non-finite and clipped samples, peak, energy, sum, the longest run of identical samples -- five flags, a
// ring of the last W hops' flags per slot and the count of flagged hops in it, and the score passed on or replaced by NaN.
// One workgroup of 256 threads per row, one launch per push, rows independent, no atomics:
//   1. thread t owns elements 1024 tile + 4 t + c of every tile (one dwordx4 load where the row is 16-byte aligned and the
//      four are inside the hop, element loads otherwise; past the hop the element is +0.0).  It accumulates q_e[c] += x * x
//      and q_s[c] += x in ascending tile order, counts non-finite and clipped samples, takes the peak as an integer max over
//      the bits of |x|, and folds its elements in stream order into a run summary (QRun).  Per tile the summaries are joined
//      across the wave (shuffle-down over ADJACENT segments: w = 1, 2, .. 32, the join is not commutative) and the four
//      wave summaries through LDS onto thread 0's running summary of the hop;
//   2. r = (q0 + q1) + (q2 + q3); the tree's w = 128 and w = 64 steps through LDS, w <= 32 by shuffle-down in wave 0.
//      Contraction is off in this kernel: every sum is one correctly rounded fp32 add of one correctly rounded product;
//   3. thread 0 joins the hop's summary to the carried (last, run), sets the flags and stores the ring entry; the 256
//      threads count the flagged entries of hops max(1, k - W + 1)..k; thread 0 writes state, totals, meas and out.
// ---------------------------------------------------------------------------------
constexpr int QUALITY_MAX_ROWS = 8192;
constexpr int QUALITY_MAX_W = 1024;         // ring entries per slot (include/afx.h states it)
constexpr int QUALITY_MAX_HOP = 1 << 24;    // samples of a hop: element indices and run lengths inside a hop stay far below 2^31
constexpr int QUALITY_N_MAX = 0x7fffffff;
constexpr int QUALITY_QNAN = 0x7fc00000;

struct QualityArgs {
  const float* x;        // (A, hop) samples at a row stride of `stride` floats
  long long stride;
  const int* hdr;        // (A, 2): slot, hop index k
  const int* scores;     // the bits of the inner scores at a stride of `sstride` words, or nullptr
  int sstride;
  unsigned char* ring;   // (S, W) flags of hop j at (j - 1) mod W
  int* state;            // (S, 3): bits of the newest sample, run, bad
  int* totals;           // (S, 6): hops, hops with each flag
  int* meas;             // (A, 8)
  int* out;              // (A,) bits of the scores passed on, or nullptr
  int A, hop, S, W, vec;
  float clip, e_quiet, dc;
  int clip_count, flat_run, mask, max_bad, abstain;
};

// the runs of identical words of a segment of the stream: its length, first and last word, the lengths of the run it
// starts with and of the run it ends with, and the longest run inside it.  len == 0: the empty segment.
struct QRun {
  int len;
  unsigned first, last;
  int pre, suf, best;
};

// segment a followed by segment b (associative, not commutative)
__device__ __forceinline__ QRun qrun_join(const QRun& a, const QRun& b) {
  if (a.len == 0) return b;
  if (b.len == 0) return a;
  const bool j = a.last == b.first;
  QRun r;
  r.len = a.len + b.len;
  r.first = a.first;
  r.last = b.last;
  r.pre = j && a.pre == a.len ? a.len + b.pre : a.pre;
  r.suf = j && b.suf == b.len ? b.len + a.suf : b.suf;
  r.best = max(max(a.best, b.best), j ? a.suf + b.pre : 0);
  return r;
}

__device__ __forceinline__ int quality_sat_inc(int v, int by) { return v > QUALITY_N_MAX - by ? QUALITY_N_MAX : v + by; }

__global__ __launch_bounds__(256) void quality_kernel(QualityArgs a) {
#pragma clang fp contract(off)
  __shared__ float s_e[256], s_s[256];
  __shared__ int s_cnt[4][3];
  __shared__ int s_run[2][4][6];
  __shared__ int s_flags, s_bad[4];
  const int row = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int slot = a.hdr[2 * row], k = a.hdr[2 * row + 1];
  const int sbits = a.scores ? a.scores[(long long)row * a.sstride] : 0;
  if (!(slot >= 0 && slot < a.S && k >= 1)) {  // (the same for every thread of the workgroup: no barrier is passed by some)
    if (tid < 8) a.meas[8ll * row + tid] = -1;
    if (tid == 0 && a.out) a.out[row] = sbits;
    return;
  }
  const float* x = a.x + (long long)row * a.stride;
  const int tiles = (a.hop + 1023) >> 10;
  float qe[4], qs[4];
  int nonfinite = 0, clipped = 0, peak = 0;  // (peak: the bits of the largest |x| that is not a NaN; they order as integers)
  QRun acc{0, 0u, 0u, 0, 0, 0};              // thread 0: the tiles taken so far
  for (int t = 0; t < tiles; ++t) {
    const int i0 = (t << 10) + 4 * tid;
    const int n = min(max(a.hop - i0, 0), 4);
    float v[4];
    if (a.vec && n == 4) {
      const float4 f = *reinterpret_cast<const float4*>(x + i0);
      v[0] = f.x, v[1] = f.y, v[2] = f.z, v[3] = f.w;
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) v[c] = c < n ? x[i0 + c] : 0.f;
    }
    QRun r{0, 0u, 0u, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float sq = v[c] * v[c];
      if (t == 0) {
        qe[c] = sq;
        qs[c] = v[c];
      } else {
        qe[c] = qe[c] + sq;
        qs[c] = qs[c] + v[c];
      }
      if (c < n) {
        const unsigned b = __float_as_uint(v[c]), ab = b & 0x7fffffffu;
        nonfinite += (b & 0x7f800000u) == 0x7f800000u;
        clipped += fabsf(v[c]) >= a.clip;
        if (ab <= 0x7f800000u) peak = max(peak, (int)ab);
        r = qrun_join(r, QRun{1, b, b, 1, 1, 1});
      }
    }
    for (int w = 1; w < 64; w <<= 1) {  // lane l (a multiple of 2 w) holds lanes l .. l + w - 1 and takes l + w .. l + 2 w - 1
      QRun o;
      o.len = __shfl_down(r.len, w);
      o.first = __shfl_down(r.first, w);
      o.last = __shfl_down(r.last, w);
      o.pre = __shfl_down(r.pre, w);
      o.suf = __shfl_down(r.suf, w);
      o.best = __shfl_down(r.best, w);
      r = qrun_join(r, o);
    }
    int* sr = s_run[t & 1][wave];
    if (lane == 0) sr[0] = r.len, sr[1] = (int)r.first, sr[2] = (int)r.last, sr[3] = r.pre, sr[4] = r.suf, sr[5] = r.best;
    __syncthreads();  // (one barrier per tile: tile t + 1 writes the other half, tile t + 2 comes after thread 0 passed t + 1's)
    if (tid == 0) {
      for (int w = 0; w < 4; ++w) {
        const int* p = s_run[t & 1][w];
        acc = qrun_join(acc, QRun{p[0], (unsigned)p[1], (unsigned)p[2], p[3], p[4], p[5]});
      }
    }
  }
  float re = (qe[0] + qe[1]) + (qe[2] + qe[3]);
  float rs = (qs[0] + qs[1]) + (qs[2] + qs[3]);
  for (int w = 32; w >= 1; w >>= 1) {
    nonfinite += __shfl_down(nonfinite, w);
    clipped += __shfl_down(clipped, w);
    peak = max(peak, __shfl_down(peak, w));
  }
  if (lane == 0) s_cnt[wave][0] = nonfinite, s_cnt[wave][1] = clipped, s_cnt[wave][2] = peak;
  s_e[tid] = re;
  s_s[tid] = rs;
  __syncthreads();
  if (tid < 128) {
    re = re + s_e[tid + 128];
    rs = rs + s_s[tid + 128];
    if (tid >= 64) s_e[tid] = re, s_s[tid] = rs;  // (entries 64..127 were read by nobody in this step)
  }
  __syncthreads();
  if (tid < 64) {
    re = re + s_e[tid + 64];
    rs = rs + s_s[tid + 64];
    for (int w = 32; w >= 1; w >>= 1) {  // lanes l < w take r[l + w]: the lanes the next step reads
      const float oe = __shfl_down(re, w), os = __shfl_down(rs, w);
      re = re + oe;
      rs = rs + os;
    }
  }
  int flags = 0, longest = 0, run1 = 0;
  if (tid == 0) {
    nonfinite = s_cnt[0][0] + s_cnt[1][0] + s_cnt[2][0] + s_cnt[3][0];
    clipped = s_cnt[0][1] + s_cnt[1][1] + s_cnt[2][1] + s_cnt[3][1];
    peak = max(max(s_cnt[0][2], s_cnt[1][2]), max(s_cnt[2][2], s_cnt[3][2]));
    const int* st = a.state + 3ll * slot;
    const unsigned last = (unsigned)st[0];
    const long long run = st[1];  // (0 for a new stream: joining it to the first sample adds nothing)
    const bool j = acc.first == last;
    longest = max(acc.best, j ? (int)min(run + acc.pre, (long long)QUALITY_N_MAX) : 0);
    run1 = j && acc.pre == acc.len ? (int)min(run + acc.len, (long long)QUALITY_N_MAX) : acc.suf;
    flags = (nonfinite > 0 ? 1 : 0) | (clipped >= a.clip_count ? 2 : 0) | (longest >= a.flat_run ? 4 : 0) |
            (re < a.e_quiet ? 8 : 0) | (fabsf(rs) > a.dc ? 16 : 0);
    a.ring[(long long)slot * a.W + (k - 1) % a.W] = (unsigned char)flags;
    s_flags = flags;
  }
  __syncthreads();
  {
    const int newest = s_flags, n = min(k, a.W);  // hops k, k - 1, .., k - n + 1: never before the session's first
    const unsigned char* rg = a.ring + (long long)slot * a.W;
    int bad = 0;
    for (int i = tid; i < n; i += 256) {
      const int f = i == 0 ? newest : rg[(k - 1 - i) % a.W];
      bad += (f & a.mask) != 0;
    }
    for (int w = 32; w >= 1; w >>= 1) bad += __shfl_down(bad, w);
    if (lane == 0) s_bad[wave] = bad;
  }
  __syncthreads();
  if (tid == 0) {
    const int bad = s_bad[0] + s_bad[1] + s_bad[2] + s_bad[3];
    int* st = a.state + 3ll * slot;
    st[0] = (int)acc.last, st[1] = run1, st[2] = bad;
    int* tot = a.totals + 6ll * slot;
    tot[0] = quality_sat_inc(tot[0], 1);
#pragma unroll
    for (int b = 0; b < 5; ++b) tot[1 + b] = quality_sat_inc(tot[1 + b], (flags >> b) & 1);
    int* m = a.meas + 8ll * row;
    m[0] = flags, m[1] = nonfinite, m[2] = clipped, m[3] = longest;
    m[4] = re != re ? QUALITY_QNAN : __float_as_int(re);  // (a NaN sum is recorded as THE quiet NaN: IEEE fixes no payload)
    m[5] = rs != rs ? QUALITY_QNAN : __float_as_int(rs);
    m[6] = peak, m[7] = bad;
    if (a.out) a.out[row] = bad <= a.max_bad || !a.abstain ? sbits : QUALITY_QNAN;
  }
}

const char* launch_quality(const float* x, long long stride, int A, int hop, const int* hdr, const float* scores, int sstride,
                           float clip, int clip_count, int flat_run, float e_quiet, float dc, int mask, int max_bad, int abstain,
                           unsigned char* ring, int W, int* state, int* totals, int S, int* meas, float* out, hipStream_t s) {
  if (!x || !hdr || !ring || !state || !totals || !meas) return "quality: null argument";
  if (scores && (!out || sstride < 1)) return "quality: scores need an output and a stride of at least 1";
  if (A <= 0 || A > QUALITY_MAX_ROWS) return "quality: 1 to 8192 rows";
  if (hop <= 0 || hop > QUALITY_MAX_HOP) return "quality: a hop of 1 to 2^24 samples";
  if (stride < hop) return "quality: a row stride of at least the hop";
  if (S <= 0) return "quality: no slots";
  if (W < 1 || W > QUALITY_MAX_W) return "quality: a window of 1 to 1024 hops";
  if (!(clip > 0.f)) return "quality: clip above 0";
  if (clip_count < 1) return "quality: clip_count of at least 1";
  if (flat_run < 2) return "quality: flat_run of at least 2";
  if (!(e_quiet >= 0.f) || !(dc >= 0.f)) return "quality: the quiet and dc bounds are 0 or more";
  if (mask < 0 || mask > 31) return "quality: mask is 0 to 31";
  if (max_bad < 0) return "quality: max_bad of 0 or more";
  if (abstain != 0 && abstain != 1) return "quality: abstain is 0 or 1";
  QualityArgs a{};
  a.x = x; a.stride = stride; a.hdr = hdr; a.scores = reinterpret_cast<const int*>(scores); a.sstride = scores ? sstride : 0;
  a.ring = ring; a.state = state; a.totals = totals; a.meas = meas; a.out = scores ? reinterpret_cast<int*>(out) : nullptr;
  a.A = A; a.hop = hop; a.S = S; a.W = W;
  a.vec = reinterpret_cast<uintptr_t>(x) % 16 == 0 && stride % 4 == 0;
  a.clip = clip; a.e_quiet = e_quiet; a.dc = dc;
  a.clip_count = clip_count; a.flat_run = flat_run; a.mask = mask; a.max_bad = max_bad; a.abstain = abstain;
  hipLaunchKernelGGL(quality_kernel, dim3(A), dim3(256), 0, s, a);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

// ---------------------------------------------------------------------------------
// Row LayerNorm (+ activation): one wave per row, C <= 1024, C % 4 == 0.  The row
// stays in registers (float4 per lane per 256-column slab), two-pass statistics in
// fp32 like torch.  Used for the conv-stack LayerNorm+GELU, every transformer /
// Conformer LayerNorm and the final encoder LayerNorm.  HBM-bound.
// ---------------------------------------------------------------------------------
template <class HT, int RPW>  // RPW rows per wave: all their loads are in flight before any is reduced
__global__ __launch_bounds__(256) void rownorm_kernel(RowNormArgs a) {
  typedef typename HT::T T;
  typedef typename HT::V4 V4;
  const int lane = threadIdx.x & 63;
  const long r0 = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * RPW;
  if (r0 >= a.rows) return;
  f32x4 v[RPW][4];
  bool live[RPW];
#pragma unroll
  for (int u = 0; u < RPW; ++u) {
    live[u] = r0 + u < a.rows;
    const float* x = a.x + (live[u] ? r0 + u : r0) * a.ldx;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int c = (it * 64 + lane) * 4;
      v[u][it] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (c < a.C) v[u][it] = *(const f32x4*)(x + c);
    }
  }
  // gamma / beta once per wave, requested before any store: on gfx9 a wait for a load that was issued after a
  // store is a wait for the store as well (one shared, out-of-order vmcnt)
  f32x4 gm[4], bt[4];
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int c = (it * 64 + lane) * 4;
    gm[it] = bt[it] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (c < a.C) {
      gm[it] = *(const f32x4*)(a.gamma + c);
      bt[it] = *(const f32x4*)(a.beta + c);
    }
  }
  const float inv = 1.0f / (float)a.C;
#pragma unroll
  for (int u = 0; u < RPW; ++u) {
    if (!live[u]) continue;  // wave-uniform
    const long r = r0 + u;
    float sum = 0.f;
#pragma unroll
    for (int it = 0; it < 4; ++it) sum += (v[u][it][0] + v[u][it][1]) + (v[u][it][2] + v[u][it][3]);
    const float mean = wave_sum(sum) * inv;
    float sq = 0.f;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int c = (it * 64 + lane) * 4;
      if (c < a.C) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          v[u][it][i] -= mean;
          sq = fmaf(v[u][it][i], v[u][it][i], sq);
        }
      }
    }
    const float var = wave_sum(sq) * inv;
    const float rstd = 1.0f / sqrtf(var + a.eps);
    // overflow guard: an operand copy that left fp16's range upstream arrives here as inf / NaN statistics (NaN fails every compare)
    // (ragged batch: a row past its utterance's own length is nobody's feature row -- its statistics are not judged)
    if (a.nonfinite && lane == 0 && !(fabsf(mean) <= 3.0e38f && var <= 3.0e38f) &&
        (!a.nf_lens || (int)(r % a.nf_rpb) < a.nf_lens[r / a.nf_rpb]))
      atomicAdd(a.nonfinite, 1);
    const long orow = (r / a.rpb) * a.o_batch_rows + (r % a.rpb) + a.o_row_off;
    // the activation branch sits OUTSIDE the element loops: inlined per element, the three activations were
    // 3 k of this kernel's 3.8 k instructions (every LayerNorm of the two models is activation-free)
    auto emit = [&](auto with_act) {
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const int c = (it * 64 + lane) * 4;
        if (c < a.C) {
          const f32x4 g = gm[it], b = bt[it];
          f32x4 y;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            y[i] = fmaf(v[u][it][i] * rstd, g[i], b[i]);
            if (decltype(with_act)::value) y[i] = apply_act(y[i], a.act);
          }
          if (a.out_f) *(f32x4*)(a.out_f + orow * a.ldo_f + c) = y;
          if (a.out_h) {
            if (std::is_same<T, float>::value && a.oh_pairs) {  // split precision: the next product's A operand, pair form
              f16x4 hi, lo;
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                const float sv = y[i] * a.oh_scale;
                hi[i] = (_Float16)sv;
                lo[i] = (_Float16)(sv - (float)hi[i]);
              }
              _Float16* hp = (_Float16*)a.out_h + orow * (2 * a.ldo_h) + s3_pair_index(c);
              *(f16x4*)hp = hi;
              *(f16x4*)(hp + 32) = lo;
            } else {
              V4 h;
#pragma unroll
              for (int i = 0; i < 4; ++i) h[i] = (T)y[i];
              *(V4*)((T*)a.out_h + orow * a.ldo_h + c) = h;
            }
          }
        }
      }
    };
    if (a.act == ACT_NONE) emit(std::false_type{});
    else emit(std::true_type{});
  }
}

const char* launch_rownorm(const RowNormArgs& a, int dtype, hipStream_t s) {
  if (a.rows <= 0 || a.C <= 0 || a.C > 1024 || a.C % 4) return "rownorm: need 0 < C <= 1024, C % 4 == 0";
  if (!a.out_f && !a.out_h) return "rownorm: no output";
  // a lane reads and writes 4 columns at a time: 16 bytes of an fp32 row, 8 bytes of a half row
  if (((size_t)a.x & 15) || (a.ldx & 3) || ((size_t)a.gamma & 15) || ((size_t)a.beta & 15))
    return "rownorm: input rows must start on 16-byte boundaries (x, gamma, beta 16-byte aligned; ldx % 4 == 0)";
  if (a.out_f && (((size_t)a.out_f & 15) || (a.ldo_f & 3))) return "rownorm: fp32 output rows must start on 16-byte boundaries (out_f 16-byte aligned, ldo_f % 4 == 0)";
  if (a.out_h && (((size_t)a.out_h & (dtype == DT_FP32 || dtype == DT_FP16X3 ? 15 : 7)) || (a.ldo_h & 3)))
    return "rownorm: operand-type output rows must start on the store's boundary (halfs: out_h 8-byte aligned, fp32: 16-byte; ldo_h % 4 == 0)";
  // two rows per wave once there are enough rows to keep 8+ waves on every CU; below that (the teacher's
  // 16 x 199 rows) one row per wave = twice the waves in flight, which is what this latency-bound size lacks
  if (a.rows >= 16384) {
    AFX_DISPATCH_HT(dtype, hipLaunchKernelGGL((rownorm_kernel<HT, 2>), dim3((a.rows + 7) / 8), dim3(256), 0, s, a));
  } else {
    AFX_DISPATCH_HT(dtype, hipLaunchKernelGGL((rownorm_kernel<HT, 1>), dim3((a.rows + 3) / 4), dim3(256), 0, s, a));
  }
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

// ---------------------------------------------------------------------------------
// zero the time-padding rows of the positional-conv operand buffer (B, pf+T+pb, C)
// ---------------------------------------------------------------------------------
// (C counts 2-byte units: an fp32 buffer passes 2 x its channel count)
__global__ void zero_pad_rows_kernel(uint16_t* buf, int T, int C, int pf, int pb, const int* __restrict__ lens) {
  const int b = blockIdx.y;
  const int keep = lens ? lens[b] : T;  // ragged batch: the frames past this utterance's own length count as padding
  const int rows = pf + pb + (T - keep);
  const long per = (long)(pf + T + pb) * C;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < (long)rows * C / 8; i += (long)gridDim.x * blockDim.x) {
    const long e = i * 8;
    int r = (int)(e / C);
    const int c = (int)(e % C);
    if (r >= pf) r += keep;
    *(u32x4*)(buf + b * per + (long)r * C + c) = u32x4{0u, 0u, 0u, 0u};
  }
}
const char* launch_zero_pad_rows(void* buf_h, int B, int T, int C, int pf, int pb, int dtype, hipStream_t s, const int* lens) {
  if (C % 8) return "zero_pad_rows: C % 8 != 0";
  if (dtype == DT_FP32) C *= 2;
  hipLaunchKernelGGL(zero_pad_rows_kernel, dim3(32, B), dim3(256), 0, s, (uint16_t*)buf_h, T, C, pf, pb, lens);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

// ---------------------------------------------------------------------------------
// weight packing (one-off): fp32 checkpoint layouts -> K-contiguous operand rows
// ---------------------------------------------------------------------------------
template <class HT>
__global__ void pack_linear_kernel(const float* w, int N, int K, int Kpad, typename HT::T* out) {
  const long total = (long)N * Kpad;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int n = (int)(i / Kpad), k = (int)(i % Kpad);
    out[i] = (typename HT::T)(k < K ? w[(long)n * K + k] : 0.f);
  }
}
const char* launch_pack_linear(const float* w, int N, int K, int Kpad, void* out_h, int dtype, hipStream_t s) {
  const int blocks = (int)min((long)4096, ((long)N * Kpad + 255) / 256);
  AFX_DISPATCH_HT(dtype, hipLaunchKernelGGL(pack_linear_kernel<HT>, dim3(blocks), dim3(256), 0, s, w, N, K, Kpad,
                                            (HT::T*)out_h));
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

// Conv1d weight [N][Cin][k] -> [N][j*Cin + c]: tap-major K so that, with channel-last
// activations, a conv row is one contiguous slice of the input.
template <class HT>
__global__ void pack_conv_kernel(const float* w, int N, int Cin, int k, typename HT::T* out) {
  const long total = (long)N * Cin * k;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int n = (int)(i / ((long)Cin * k));
    const int rem = (int)(i % ((long)Cin * k));
    const int j = rem / Cin, c = rem % Cin;
    out[i] = (typename HT::T)w[((long)n * Cin + c) * k + j];
  }
}
const char* launch_pack_conv(const float* w, int N, int Cin, int k, void* out_h, int dtype, hipStream_t s) {
  const int blocks = (int)min((long)4096, ((long)N * Cin * k + 255) / 256);
  AFX_DISPATCH_HT(dtype, hipLaunchKernelGGL(pack_conv_kernel<HT>, dim3(blocks), dim3(256), 0, s, w, N, Cin, k,
                                            (HT::T*)out_h));
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

// Positional conv: weight_v [C][cpg][k] (+ weight_g [k], weight-norm over dims (0,1))
// -> [C][j*cpg + c] with the per-tap scale g[j] / ||v[:,:,j]|| folded in.
__global__ void posconv_norm_kernel(const float* v, int C, int cpg, int k, float* norm) {
  const int j = blockIdx.x;
  float s = 0.f;
  for (long i = threadIdx.x; i < (long)C * cpg; i += blockDim.x) {
    const float x = v[i * k + j];
    s = fmaf(x, x, s);
  }
  __shared__ float red[4];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) norm[j] = sqrtf(red[0] + red[1] + red[2] + red[3]);
}
template <class HT>
__global__ void pack_posconv_kernel(const float* v, const float* g, const float* norm, int C, int cpg, int k,
                                    typename HT::T* out) {
  const long total = (long)C * cpg * k;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int o = (int)(i / ((long)cpg * k));
    const int rem = (int)(i % ((long)cpg * k));
    const int j = rem / cpg, c = rem % cpg;
    float x = v[((long)o * cpg + c) * k + j];
    if (g) x = x * g[j] / norm[j];
    out[i] = (typename HT::T)x;
  }
}
const char* launch_pack_posconv(const float* v, const float* g, int C, int cpg, int k, float* norm_tmp, void* out_h,
                                int dtype, hipStream_t s) {
  if (g) hipLaunchKernelGGL(posconv_norm_kernel, dim3(k), dim3(256), 0, s, v, C, cpg, k, norm_tmp);
  const int blocks = (int)min((long)4096, ((long)C * cpg * k + 255) / 256);
  AFX_DISPATCH_HT(dtype, hipLaunchKernelGGL(pack_posconv_kernel<HT>, dim3(blocks), dim3(256), 0, s, v, g, norm_tmp, C,
                                            cpg, k, (HT::T*)out_h));
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

// ---- split precision (DT_FP16X3) operand preparation --------------------------------------------------------------------
// One workgroup per weight row: the row is read whole (registers -> LDS) before anything is written, so its pair form
// (afx_kernels.h: hi / lo halves interleaved in groups of 32) can take the place of the fp32 row it was made from.
__global__ __launch_bounds__(256) void split_weight_rows_kernel(float* w, int K, float* row_scale) {
  extern __shared__ float srow[];
  float* row = w + (long)blockIdx.x * K;
  float mx = 0.f;
  for (int k = threadIdx.x; k < K; k += 256) {
    const float v = row[k];
    srow[k] = v;
    mx = fmaxf(mx, fabsf(v));
  }
  __shared__ float red[4];
  mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  // 2^e with mx * 2^e in [8192, 16384): hi parts are far from fp16's overflow, lo parts of typical entries far from its subnormals
  int e = 0;
  if (mx > 0.f && mx < 3.0e38f) {
    int ex;
    (void)frexpf(mx, &ex);  // mx = f * 2^ex, f in [0.5, 1)
    e = 14 - ex;
    e = e > 100 ? 100 : (e < -100 ? -100 : e);
  }
  const float sc = ldexpf(1.0f, e);
  __syncthreads();  // (every thread has read its part of the row: the pair form overwrites it)
  _Float16* out = (_Float16*)row;
  for (int k = threadIdx.x; k < K; k += 256) {
    const float v = srow[k] * sc;
    const _Float16 h = (_Float16)v;
    const long o = s3_pair_index(k);
    out[o] = h;
    out[o + 32] = (_Float16)(v - (float)h);
  }
  if (threadIdx.x == 0) row_scale[blockIdx.x] = ldexpf(1.0f, -e);
}
const char* launch_split_weight_rows(void* w, int N, int K, float* row_scale, hipStream_t s) {
  if (K > 12288 || K % 32) return "split_weight_rows: rows of at most 12288 elements, whole 32-element groups";
  static LdsLimit lim;
  if (hipError_t e = lim.ensure((const void*)split_weight_rows_kernel, K * 4 + 64); e != hipSuccess) return hipGetErrorString(e);
  hipLaunchKernelGGL(split_weight_rows_kernel, dim3(N), dim3(256), (size_t)K * 4, s, (float*)w, K, row_scale);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

// fp32 values -> their pair form: a thread turns 8 consecutive values (inside one 32-element group) into 16 B of hi and 16 B of lo halves
__global__ __launch_bounds__(256) void split_pairs_kernel(const float* __restrict__ x, long n8, _Float16* __restrict__ out, float scale) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long)gridDim.x * 256) {
    const long o = i * 8;
    const f32x4 a = *(const f32x4*)(x + o), b = *(const f32x4*)(x + o + 4);
    f16x8 h, l;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float va = a[r] * scale, vb = b[r] * scale;
      h[r] = (_Float16)va;
      h[4 + r] = (_Float16)vb;
      l[r] = (_Float16)(va - (float)h[r]);
      l[4 + r] = (_Float16)(vb - (float)h[4 + r]);
    }
    _Float16* hp = out + s3_pair_index(o);
    *(f16x8*)hp = h;
    *(f16x8*)(hp + 32) = l;
  }
}
const char* launch_split_pairs(const float* x, long n, void* pairs, float scale, hipStream_t s) {
  if (n <= 0) return nullptr;
  if (((size_t)x & 15) || ((size_t)pairs & 15) || (n & 31)) return "split_pairs: whole groups of 32 elements, 16-byte aligned";
  const long n8 = n / 8;
  const int blocks = (int)min((long)8192, (n8 + 255) / 256);
  hipLaunchKernelGGL(split_pairs_kernel, dim3(blocks), dim3(256), 0, s, x, n8, (_Float16*)pairs, scale);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

}  // namespace afx
