// AASIST graph-attention back-end on gfx950, all fp32.
//
// Why fp32 everywhere: GraphPool's top-k is discontinuous, so the head is kept free
// of operand rounding.  The FLOP-heavy part (the 2-D residual encoder, ~1.2 GFLOP per
// utterance) still runs on the matrix cores through v_mfma_f32_16x16x4_f32, which is
// bit-for-bit an fp32 fma chain (cdna guide, "FP32-input MFMA").
//
// Data layout: encoder activations are channel-last in a zero-padded image
// (B, HP, WP, C), logical pixel (h,w) at (h+1,w+1).  With the padding materialised a
// (kh,3) convolution of "virtual pixel" m = h*WP + w is
//     out[m][n] = sum_{dh<kh} A[(m + dh*WP)*C : +3C] . Wt[n][dh*3C : +3C]
// i.e. a GEMM whose K dimension is kh contiguous chunks -- no im2col, no bounds tests
// in the inner loop; virtual pixels that fall in the padding are masked to zero in the
// epilogue, which at the same time re-creates the zero border of the output image.
#include "afx_aasist.h"

#include <cstring>

#include "afx_common.h"

namespace afx {

// ===================================================================================
// fp32 matrix-core GEMM with chunked K (convs, 1x1 convs, the LL linear)
// ===================================================================================
struct F32GemmArgs {
  const float* A;
  long lda;            // elements between consecutive (virtual) rows
  int nch, kc;         // K = nch chunks of kc contiguous elements (kc % 16 == 0)
  long chunk_stride;   // elements between chunks of one row
  const float* W;      // [N][nch*kc]
  // split-precision form (f32s_gemm_kernel): the same weights as fp16 pairs, W = Wh + 2^-11 Wl (null: fp32 MFMA)
  const _Float16* Wh;
  const _Float16* Wl;
  int M, N;            // N = 16 * NT
  const float* bias;   // [N] or null
  const float* resid;  // indexed like out, or null
  const float* bn_scale;  // [N] or null
  const float* bn_shift;
  int post;            // 0: none  1: bn -> selu (after resid)  2: selu -> bn
  // validity mask of virtual pixels (img == 0 disables): pix = m % img; valid iff
  // pix / wp < hout && pix % wp < wd; invalid outputs are written as 0
  int img, wp, hout, wd;
  float* out;
  long ldo;
  long o_off;          // output row = m + o_off
};

// One wave = 32 rows x 16 NT columns; blockIdx.y walks column blocks of 16 NT (the launcher picks NT so that the grid
// gives every SIMD of the chip at least one wave: the LL product, M = 16 x 199 rows, was 25 workgroups before).
// Operand fragments come straight from L2 (a lane's 16 B of a row per k-step of 16: 6 loads per 32-64 MFMAs).
template <int NT>
__global__ __launch_bounds__(256) void f32_gemm_kernel(F32GemmArgs p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, kq = lane >> 4;
  const long m0 = ((long)blockIdx.x * 4 + wave) * 32;
  if (m0 >= p.M) return;
  const int n0 = blockIdx.y * NT * 16;
  const long ldw = (long)p.nch * p.kc;
  const float* arow[2];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) {
    long m = m0 + mt * 16 + r;
    m = m < p.M ? m : p.M - 1;
    arow[mt] = p.A + m * p.lda + kq * 4;
  }
  const float* wrow = p.W + (long)(n0 + r) * ldw + kq * 4;
  f32x4 acc[2][NT];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  // (Measured and dropped, profiles/r02_aasist_gemm_prefetch_ab.txt: fragments one / two k-steps ahead in rotating
  // register sets -- 38.2 / 42.8 us against 36.3 us for this plain loop on the (2,3) convs: two to four waves per SIMD
  // already cover each other's L2 round trips, the extra registers only cost occupancy.)
  for (int ch = 0; ch < p.nch; ++ch) {
    const long ao = (long)ch * p.chunk_stride;
    const long wo = (long)ch * p.kc;
    for (int k0 = 0; k0 < p.kc; k0 += 16) {
      f32x4 a[2], b[NT];
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) a[mt] = *(const f32x4*)(arow[mt] + ao + k0);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) b[nt] = *(const f32x4*)(wrow + (long)nt * 16 * ldw + wo + k0);
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt)
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(b[nt][s], a[mt][s], acc[mt][nt], 0, 0, 0);
    }
  }
  // operands swapped: lane holds out[m = .. + (lane&15)][n = n0 + 16nt + 4*(lane>>4) + 0..3]
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) {
    const long m = m0 + mt * 16 + r;
    if (m >= p.M) continue;
    bool valid = true;
    if (p.img) {
      const int pix = (int)(m % p.img);
      valid = (pix / p.wp < p.hout) && (pix % p.wp < p.wd);
    }
    const long orow = (m + p.o_off) * p.ldo;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int n = n0 + nt * 16 + kq * 4;
      f32x4 v = acc[mt][nt];
      if (p.bias) v += *(const f32x4*)(p.bias + n);
      if (p.resid) v += *(const f32x4*)(p.resid + orow + n);
      if (p.post == 1) {
        const f32x4 sc = *(const f32x4*)(p.bn_scale + n), sh = *(const f32x4*)(p.bn_shift + n);
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = selu(fmaf(v[i], sc[i], sh[i]));
      } else if (p.post == 2) {
        const f32x4 sc = *(const f32x4*)(p.bn_scale + n), sh = *(const f32x4*)(p.bn_shift + n);
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = fmaf(selu(v[i]), sc[i], sh[i]);
      }
      if (!valid) v = f32x4{0.f, 0.f, 0.f, 0.f};
      *(f32x4*)(p.out + orow + n) = v;
    }
  }
}

// ===================================================================================
// The same product at fp32 ACCURACY on the fp16 matrix pipe (16x the rate of the fp32 MFMA).
// Every fp32 operand is split into two fp16 halves, x = xh + 2^-11 xl with xh = fp16(x), xl = fp16((x - xh) 2^11):
// the residue x - xh is exact in fp32, the scaling keeps xl a NORMAL fp16 number for every |x| > 6e-5 (unscaled, the
// low half of anything below 0.125 would be subnormal) and xh + 2^-11 xl carries 22 mantissa bits.  Then
//     a w  =  ah wh  +  2^-11 (ah wl + al wh)  +  O(2^-22 a w)
// with each fp16 x fp16 product exact in the MFMA's fp32 accumulation.  Three v_mfma_f32_16x16x32_f16 (48 cycles per
// 16 x 16 x 32 block) replace eight v_mfma_f32_16x16x4_f32 (256 cycles); the main and the correction terms keep their
// own fp32 accumulators and meet once at the end.  Weights are split once at load time, activations in registers
// (two cvt, a subtract and a multiply per element).  Relative error of a dot product ~3e-7: the same order as the
// fp32 kernel's own summation-order noise against the CPU reference (both are "fp32" only up to that).
// The engine's exact mode (dtype fp32) and the stand-alone module entry points keep the true-fp32 kernel above.
// ===================================================================================
typedef __attribute__((ext_vector_type(8))) _Float16 h16x8;
template <int NT>
__global__ __launch_bounds__(256) void f32s_gemm_kernel(F32GemmArgs p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, kq = lane >> 4;
  const long m0 = ((long)blockIdx.x * 4 + wave) * 32;
  if (m0 >= p.M) return;
  const int n0 = blockIdx.y * NT * 16;
  const long ldw = (long)p.nch * p.kc;
  const float* arow[2];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) {
    long m = m0 + mt * 16 + r;
    m = m < p.M ? m : p.M - 1;
    arow[mt] = p.A + m * p.lda + kq * 8;
  }
  const long woff = (long)(n0 + r) * ldw + kq * 8;
  f32x4 acc[2][NT], cor[2][NT];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = cor[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int ch = 0; ch < p.nch; ++ch) {
    const long ao = (long)ch * p.chunk_stride;
    const long wo = (long)ch * p.kc;
    for (int k0 = 0; k0 < p.kc; k0 += 32) {
      f32x4 x[2][2];
      h16x8 wh[NT], wl[NT];
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        x[mt][0] = *(const f32x4*)(arow[mt] + ao + k0);
        x[mt][1] = *(const f32x4*)(arow[mt] + ao + k0 + 4);
      }
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        wh[nt] = *(const h16x8*)(p.Wh + woff + (long)nt * 16 * ldw + wo + k0);
        wl[nt] = *(const h16x8*)(p.Wl + woff + (long)nt * 16 * ldw + wo + k0);
      }
      h16x8 ah[2], al[2];
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float v = x[mt][i >> 2][i & 3];
          const _Float16 hi = (_Float16)v;
          ah[mt][i] = hi;
          al[mt][i] = (_Float16)((v - (float)hi) * 2048.0f);
        }
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[nt], ah[mt], acc[mt][nt], 0, 0, 0);
          cor[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[nt], ah[mt], cor[mt][nt], 0, 0, 0);
          cor[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[nt], al[mt], cor[mt][nt], 0, 0, 0);
        }
    }
  }
  // operands swapped: lane holds out[m = .. + (lane&15)][n = n0 + 16nt + 4*(lane>>4) + 0..3]
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) {
    const long m = m0 + mt * 16 + r;
    if (m >= p.M) continue;
    bool valid = true;
    if (p.img) {
      const int pix = (int)(m % p.img);
      valid = (pix / p.wp < p.hout) && (pix % p.wp < p.wd);
    }
    const long orow = (m + p.o_off) * p.ldo;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int n = n0 + nt * 16 + kq * 4;
      f32x4 v = acc[mt][nt] + cor[mt][nt] * (1.0f / 2048.0f);
      if (p.bias) v += *(const f32x4*)(p.bias + n);
      if (p.resid) v += *(const f32x4*)(p.resid + orow + n);
      if (p.post == 1) {
        const f32x4 sc = *(const f32x4*)(p.bn_scale + n), sh = *(const f32x4*)(p.bn_shift + n);
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = selu(fmaf(v[i], sc[i], sh[i]));
      } else if (p.post == 2) {
        const f32x4 sc = *(const f32x4*)(p.bn_scale + n), sh = *(const f32x4*)(p.bn_shift + n);
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = fmaf(selu(v[i]), sc[i], sh[i]);
      }
      if (!valid) v = f32x4{0.f, 0.f, 0.f, 0.f};
      *(f32x4*)(p.out + orow + n) = v;
    }
  }
}

// ===================================================================================
// The (2,3) / (1,3) / 1x1 convs of the residual encoder, LDS-staged.  f32_gemm_kernel / f32s_gemm_kernel fetch every
// operand fragment straight from L2 in 64-byte pieces (16 rows x 64 B per load instruction) and every wave re-reads
// the whole weight matrix: 230 MB of L2 traffic in fragment-shaped loads per conv -- that, not the matrix pipe, is what
// they run at (the split-precision form cut the MFMA work 5x and the time by 7 %).  Here a persistent workgroup keeps
// the split weights (hi | lo fp16, rows padded by 16 B) in LDS for its whole life and stages, per 64 output pixels, the
// 2 x 66 input pixels they read (channel-last, so a (kh,3) conv reads kh contiguous runs of pixels) with coalesced
// 16-byte loads, the next tile's pixels travelling through registers under the current tile's MFMAs.  A fragments come
// from LDS (pixel rows padded by 16 B: conflict-free across the 16 rows of a fragment), are split hi / lo in
// registers, and feed the same three MFMAs per block as f32s_gemm_kernel.
// ===================================================================================
constexpr int ACV_TM = 64;  // output pixels per workgroup step
// 8 waves: wave w owns output pixels 16 (w & 3) .. +15 and the column half (w >> 2) of the N outputs, so every SIMD
// holds two waves (one workgroup per CU: the weights of the 64 -> 64 (2,3) conv are 100 KB of LDS).  The staged pixels
// are split into their fp16 hi / lo halves ONCE, while they are written to LDS (each is then read by kh x 3 taps and
// two column waves): the inner loop is LDS fragment reads and MFMAs only.
constexpr int ACV_PAD = 16;  // halfs of padding per LDS row (32 B)
template <int NT>
__global__ __launch_bounds__(512) void aas_conv_kernel(F32GemmArgs p, int C, int taps, int cpo, int ntiles) {
  static_assert(NT % 2 == 0, "two column halves");
  constexpr int NTW = NT / 2;  // 16-column tiles per wave
  extern __shared__ __attribute__((aligned(16))) char acv_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, kq = lane >> 4;
  constexpr int N = NT * 16;
  // LDS rows (weights: K halfs, pixels: C halfs; both multiples of 32) are padded by 32 B: a row stride of 32 (mod 64) bytes
  // is what the lane groups of ds_read_b128 -- {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, ... (MI355X_MICROARCH.md, LDS) --
  // read without a bank conflict when lane l takes row l & 15, 16-byte piece l >> 4.  Round 3's 16 B of padding (stride 16
  // mod 64) put two addresses on a bank in every group: SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE 0.41 - 0.47 on these kernels.
  const int K = p.nch * p.kc, Kp = K + ACV_PAD;            // halfs per weight row in LDS
  const int Cp = C + ACV_PAD, SP = ACV_TM + taps - 1;      // halfs per pixel in LDS; pixels per slab
  _Float16* wh = (_Float16*)acv_lds;                 // [N][Kp]
  _Float16* wl = wh + (long)N * Kp;                  // [N][Kp]
  _Float16* sh = wl + (long)N * Kp;                  // [nch][SP][Cp]  hi halves of the staged pixels
  _Float16* sl = sh + (long)p.nch * SP * Cp;         // [nch][SP][Cp]  lo halves (scaled by 2^11)
  // ---- weights: once per workgroup; ALL of a thread's loads go out before its first LDS write (left as a plain
  // loop the copy was six dependent L2 round trips: a third of the kernel's time at three tiles per workgroup) -------
  {
    constexpr int WPMAX = 6;  // 16-byte pieces per thread and array (64 x 384 / 8 / 512 = 6; the launcher checks)
    h16x8 th[WPMAX], tl[WPMAX];
    const int npw = N * (K / 8);
#pragma unroll
    for (int u = 0; u < WPMAX; ++u) {
      const int i = tid + u * 512;
      if (i < npw) {
        th[u] = *(const h16x8*)(p.Wh + (long)i * 8);
        tl[u] = *(const h16x8*)(p.Wl + (long)i * 8);
      }
    }
#pragma unroll
    for (int u = 0; u < WPMAX; ++u) {
      const int i = tid + u * 512;
      if (i < npw) {
        const int n = i / (K / 8), c8 = i % (K / 8);
        *(h16x8*)(wh + (long)n * Kp + c8 * 8) = th[u];
        *(h16x8*)(wl + (long)n * Kp + c8 * 8) = tl[u];
      }
    }
  }
  // ---- staging plan: piece j = (chunk, pixel, 4 channels); the plan does not depend on the tile ----
  const int c4 = C / 4, npiece = p.nch * SP * c4;
  constexpr int PMAX = 5;  // pieces per thread (2 x 66 x 16 / 512 = 4.1 for C = 64; the launcher checks)
  int src_rel[PMAX], dst_off[PMAX];  // source: float offset relative to pixel m0; destination: half offset in sh / sl
  long lim_rel[PMAX];
  const long last_pix = (long)p.M - 1 + (long)cpo * (p.nch - 1) + taps - 1;  // last pixel any valid row reads
#pragma unroll
  for (int u = 0; u < PMAX; ++u) {
    const int j = tid + u * 512;
    const int jj = j < npiece ? j : 0;
    const int ch = jj / (SP * c4), rem = jj % (SP * c4), px = rem / c4, cc = rem % c4;
    src_rel[u] = ch * cpo + px;  // pixels past m0
    lim_rel[u] = cc * 4;
    dst_off[u] = j < npiece ? (ch * SP + px) * Cp + cc * 4 : -1;
  }
  f32x4 stage[PMAX];
  auto fetch = [&](int tile) {
    const long m0 = (long)tile * ACV_TM;
#pragma unroll
    for (int u = 0; u < PMAX; ++u)
      if (dst_off[u] >= 0) {
        long pix = m0 + src_rel[u];
        pix = pix < last_pix ? pix : last_pix;
        stage[u] = *(const f32x4*)(p.A + pix * C + lim_rel[u]);
      }
  };
  auto commit = [&]() {
#pragma unroll
    for (int u = 0; u < PMAX; ++u)
      if (dst_off[u] >= 0) {
        typedef __attribute__((ext_vector_type(4))) _Float16 h16x4;
        h16x4 hi, lo;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float v = stage[u][i];
          hi[i] = (_Float16)v;
          lo[i] = (_Float16)((v - (float)hi[i]) * 2048.0f);
        }
        *(h16x4*)(sh + dst_off[u]) = hi;
        *(h16x4*)(sl + dst_off[u]) = lo;
      }
  };
  // per-column vectors of this lane's outputs (n = 16 (col half, nt) + 4 kq + 0..3): loaded once
  const int nbase = (wave >> 2) * NTW * 16;
  f32x4 vb[NTW], vsc[NTW], vsh[NTW];
#pragma unroll
  for (int nt = 0; nt < NTW; ++nt) {
    const int n = nbase + nt * 16 + kq * 4;
    vb[nt] = p.bias ? *(const f32x4*)(p.bias + n) : f32x4{0.f, 0.f, 0.f, 0.f};
    vsc[nt] = p.post ? *(const f32x4*)(p.bn_scale + n) : f32x4{1.f, 1.f, 1.f, 1.f};
    vsh[nt] = p.post ? *(const f32x4*)(p.bn_shift + n) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  int tile = blockIdx.x;
  if (tile < ntiles) fetch(tile);
  const int lr = (wave & 3) * 16 + r;
  for (; tile < ntiles; tile += gridDim.x) {
    __syncthreads();  // every wave is done with the previous slab
    commit();
    __syncthreads();  // slab (and, first time round, the weights) visible
    // this tile's residual rows and the next tile's pixels are requested now and ride under this tile's MFMAs
    const long m = (long)tile * ACV_TM + lr;
    const long orow = ((m < p.M ? m : (long)p.M - 1) + p.o_off) * p.ldo;
    f32x4 res[NTW];
    if (p.resid) {
#pragma unroll
      for (int nt = 0; nt < NTW; ++nt) res[nt] = *(const f32x4*)(p.resid + orow + nbase + nt * 16 + kq * 4);
    }
    if (tile + (int)gridDim.x < ntiles) fetch(tile + gridDim.x);
    f32x4 acc[NTW], cor[NTW];
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt) acc[nt] = cor[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int ch = 0; ch < p.nch; ++ch)
      for (int tp = 0; tp < taps; ++tp) {
        const long ao = ((long)ch * SP + lr + tp) * Cp + kq * 8;
        const int kbase = ch * p.kc + tp * C;
        for (int c0 = 0; c0 < C; c0 += 32) {
          const h16x8 ah = *(const h16x8*)(sh + ao + c0), al = *(const h16x8*)(sl + ao + c0);
          h16x8 bh[NTW], bl[NTW];
#pragma unroll
          for (int nt = 0; nt < NTW; ++nt) {
            const long wo = (long)(nbase + nt * 16 + r) * Kp + kbase + c0 + kq * 8;
            bh[nt] = *(const h16x8*)(wh + wo);
            bl[nt] = *(const h16x8*)(wl + wo);
          }
#pragma unroll
          for (int nt = 0; nt < NTW; ++nt) {
            acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bh[nt], ah, acc[nt], 0, 0, 0);
            cor[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bl[nt], ah, cor[nt], 0, 0, 0);
            cor[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bh[nt], al, cor[nt], 0, 0, 0);
          }
        }
      }
    // epilogue: lane holds out[m = m0 + 16 (wave & 3) + (lane&15)][n = nbase + 16 nt + 4 (lane>>4) + 0..3]
    if (m < p.M) {
      bool valid = true;
      if (p.img) {
        const int pix = (int)(m % p.img);
        valid = (pix / p.wp < p.hout) && (pix % p.wp < p.wd);
      }
#pragma unroll
      for (int nt = 0; nt < NTW; ++nt) {
        const int n = nbase + nt * 16 + kq * 4;
        f32x4 v = acc[nt] + cor[nt] * (1.0f / 2048.0f) + vb[nt];
        if (p.resid) v += res[nt];
        if (p.post == 1) {
#pragma unroll
          for (int i = 0; i < 4; ++i) v[i] = selu(fmaf(v[i], vsc[nt][i], vsh[nt][i]));
        } else if (p.post == 2) {
#pragma unroll
          for (int i = 0; i < 4; ++i) v[i] = fmaf(selu(v[i]), vsc[nt][i], vsh[nt][i]);
        }
        if (!valid) v = f32x4{0.f, 0.f, 0.f, 0.f};
        *(f32x4*)(p.out + orow + n) = v;
      }
    }
  }
}

// test knob (afx_debug_set "aasist_conv_slots"): > 0 caps the grid at that many workgroups, so that a small problem
// walks many tiles per workgroup (the prefetch of the next tile and its clamp at last_pix); 0 = automatic
static int g_aas_conv_slots = 0;
void aasist_set_conv_slots(int v) { g_aas_conv_slots = v > 0 ? v : 0; }

// launch the LDS-staged form when the shape allows it; false = not applicable (caller falls back)
static bool try_launch_aas_conv(const F32GemmArgs& p, hipStream_t s, hipError_t* err) {
  *err = hipSuccess;
  if (!p.Wh || !p.Wl || p.lda <= 0 || p.lda % 32 || p.kc % p.lda || p.chunk_stride % p.lda) return false;
  const int C = (int)p.lda, taps = p.kc / C, cpo = (int)(p.chunk_stride / C), K = p.nch * p.kc;
  const int SP = ACV_TM + taps - 1;
  const long lds = 2L * p.N * (K + ACV_PAD) * 2 + 2L * p.nch * SP * (C + ACV_PAD) * 2;
  if (lds > 160 * 1024 || (long)p.nch * SP * (C / 4) > 5 * 512 || (long)p.N * (K / 8) > 6 * 512) return false;
  const int ntiles = (int)((p.M + ACV_TM - 1) / ACV_TM);
  static int n_cu_of[kMaxDevices] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) { *err = hipErrorInvalidDevice; return true; }
  if (!n_cu_of[dev] && hipDeviceGetAttribute(&n_cu_of[dev], hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) { *err = hipErrorUnknown; return true; }
  const int per_cu = (int)((160 * 1024) / lds) > 2 ? 2 : (int)((160 * 1024) / lds);  // 512-thread workgroups
  int slots = n_cu_of[dev] * (per_cu < 1 ? 1 : per_cu);
  if (g_aas_conv_slots > 0 && g_aas_conv_slots < slots) slots = g_aas_conv_slots;
  dim3 grid(ntiles < slots ? ntiles : slots);
  static LdsLimit lim[3];
#define AFX_ACV(IDX, NTv)                                                                                 \
  do {                                                                                                    \
    *err = lim[IDX].ensure((const void*)aas_conv_kernel<NTv>, (int)lds);                                  \
    if (*err == hipSuccess) hipLaunchKernelGGL(aas_conv_kernel<NTv>, grid, dim3(512), (size_t)lds, s, p, C, taps, cpo, ntiles); \
  } while (0)
  if (p.N == 32) AFX_ACV(0, 2);
  else if (p.N == 64) AFX_ACV(1, 4);
  else if (p.N == 128) AFX_ACV(2, 8);
  else return false;
#undef AFX_ACV
  if (*err == hipSuccess) *err = hipGetLastError();
  return true;
}

// fp32 weights -> (hi, 2^11-scaled lo) fp16 pair, once at load time
__global__ void split_f16_kernel(const float* __restrict__ w, long n, _Float16* __restrict__ hi, _Float16* __restrict__ lo) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float v = w[i];
    const _Float16 h = (_Float16)v;
    hi[i] = h;
    lo[i] = (_Float16)((v - (float)h) * 2048.0f);
  }
}

static const char* launch_f32_gemm(const F32GemmArgs& p, hipStream_t s) {
  if (p.kc % 16 || p.M <= 0) return "aasist gemm: chunk length must be a multiple of 16";
  if (p.N != 32 && p.N != 64 && p.N != 128) return "aasist gemm: N must be 32, 64 or 128";
  // columns per wave: as wide as possible (A rows are re-read once per column block) while the grid still gives
  // each of the chip's 1024 SIMDs a wave
  const long row_waves = (p.M + 31) / 32;
  int nt = p.N / 16;
  while (nt > 1 && row_waves * (p.N / (16 * nt)) < 1024) nt >>= 1;
  dim3 grid((unsigned)((p.M + 127) / 128), p.N / (16 * nt));
  if (p.Wh && p.Wl) {  // split-precision form on the fp16 matrix pipe
    hipError_t ce;
    if (try_launch_aas_conv(p, s, &ce)) return ce == hipSuccess ? nullptr : hipGetErrorString(ce);  // LDS-staged convs
    if (p.kc % 32 || (p.lda % 4) || (p.chunk_stride % 4)) return "aasist gemm (split precision): K chunks of 32, 16-B aligned rows";
    if (nt > 4) {  // 2 x NT x 2 accumulator tiles: keep the wave at 4 column tiles
      nt = 4;
      grid.y = p.N / 64;
    }
    switch (nt) {
      case 1: hipLaunchKernelGGL(f32s_gemm_kernel<1>, grid, dim3(256), 0, s, p); break;
      case 2: hipLaunchKernelGGL(f32s_gemm_kernel<2>, grid, dim3(256), 0, s, p); break;
      default: hipLaunchKernelGGL(f32s_gemm_kernel<4>, grid, dim3(256), 0, s, p); break;
    }
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? nullptr : hipGetErrorString(e);
  }
  switch (nt) {
    case 1: hipLaunchKernelGGL(f32_gemm_kernel<1>, grid, dim3(256), 0, s, p); break;
    case 2: hipLaunchKernelGGL(f32_gemm_kernel<2>, grid, dim3(256), 0, s, p); break;
    case 4: hipLaunchKernelGGL(f32_gemm_kernel<4>, grid, dim3(256), 0, s, p); break;
    default: hipLaunchKernelGGL(f32_gemm_kernel<8>, grid, dim3(256), 0, s, p); break;
  }
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

// ===================================================================================
// small kernels
// ===================================================================================
// models/xlsr_aasist.py:92-96: (B,T,128) -> transpose -> max_pool2d(3,3) -> BN2d(1) -> SELU,
// written as a 1-channel padded image.
__global__ void pool_bn_selu_kernel(const float* __restrict__ ll, int T, int wd, int wp, int img, float sc, float sh,
                                    float* __restrict__ out, int B, int tail, float* __restrict__ za, float* __restrict__ zb,
                                    float* __restrict__ zc, int head) {
  // Writes EVERY pixel of the 1-channel padded image (zeros on the border), so nothing has to be cleared first; the
  // extra grid row y == B zeroes the slack behind the last image and the heads of the three multi-channel images.
  const int b = blockIdx.y;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (b == B) {
    const int step = gridDim.x * blockDim.x;
    for (int i = idx; i < tail; i += step) out[(long)B * img + i] = 0.f;
    for (int i = idx; i < head; i += step) {
      za[i] = 0.f;
      zb[i] = 0.f;
      zc[i] = 0.f;
    }
    return;
  }
  if (idx >= img) return;
  const int h = idx / wp, wq = idx % wp;
  float v = 0.f;
  if (h >= 1 && h <= AAS_F && wq >= 1 && wq <= wd) {
    const int fi = h - 1, ti = wq - 1;
    float m = -INFINITY;
#pragma unroll
    for (int dt = 0; dt < 3; ++dt)
#pragma unroll
      for (int df = 0; df < 3; ++df) m = fmaxf(m, ll[((long)b * T + ti * 3 + dt) * 128 + fi * 3 + df]);
    v = selu(fmaf(m, sc, sh));
  }
  out[(long)b * img + idx] = v;
}

// zero the first `n` floats of three buffers in one launch (image heads when the channel-last layout widens)
__global__ void zero3_kernel(float* __restrict__ a, float* __restrict__ b, float* __restrict__ c, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    a[i] = 0.f;
    b[i] = 0.f;
    c[i] = 0.f;
  }
}

// first residual block (Cin = 1): conv1 (2,3) pad (1,1) -> bn2 -> selu into Y (43 rows) and
// the (1,3) downsample conv into D (42 rows).  One thread per (virtual pixel, channel).
__global__ void first_block_kernel(const float* __restrict__ x, int M, int img, int wp, int wd, const float* __restrict__ w1,
                                   const float* __restrict__ b1, const float* __restrict__ sc, const float* __restrict__ sh,
                                   const float* __restrict__ wd_, const float* __restrict__ bd, float* __restrict__ Y,
                                   float* __restrict__ D, int cout, int hin) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)M * cout) return;
  const long m = idx / cout;
  const int n = (int)(idx % cout);
  const int pix = (int)(m % img), h = pix / wp, w = pix % wp;
  float y = 0.f, d = 0.f;
  if (w < wd && h < hin + 1) {
    float a = b1[n];
#pragma unroll
    for (int dh = 0; dh < 2; ++dh)
#pragma unroll
      for (int dw = 0; dw < 3; ++dw) a = fmaf(x[m + dh * wp + dw], w1[n * 6 + dh * 3 + dw], a);
    y = selu(fmaf(a, sc[n], sh[n]));
    if (h < hin) {
      float e = bd[n];
#pragma unroll
      for (int dw = 0; dw < 3; ++dw) e = fmaf(x[m + wp + dw], wd_[n * 3 + dw], e);
      d = e;
    }
  }
  const long o = (m + wp + 1) * cout + n;
  Y[o] = y;
  D[o] = d;
}

// conv weight [cout][cin][kh][kw] -> tap-major [cout][(dh*kw + dw)*cin + c]
__global__ void pack_conv2d_kernel(const float* w, int cout, int cin, int kh, int kw, float* out) {
  const int total = cout * cin * kh * kw;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int n = i / (cin * kh * kw), rem = i % (cin * kh * kw);
    const int tap = rem / cin, c = rem % cin;
    out[i] = w[((long)n * cin + c) * kh * kw + tap];
  }
}
__global__ void bn_fold2_kernel(const float* w, const float* b, const float* m, const float* v, float eps, int n,
                                float* scale, float* shift) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const float s = w[i] / sqrtf(v[i] + eps);
    scale[i] = s;
    shift[i] = b[i] - m[i] * s;
  }
}

// models/xlsr_aasist.py:106-118: softmax-weighted pooling over time (e_S, + pos_S) and over
// frequency (e_T).  Block = 64 threads (channels); blockIdx.x < 42 -> spectral node h,
// else temporal node w.
__global__ void att_pool_kernel(const float* __restrict__ x, const float* __restrict__ wm, int img, int wp, int wd,
                                const float* __restrict__ pos_S, float* __restrict__ eS, float* __restrict__ eT) {
  const int b = blockIdx.y, c = threadIdx.x;
  const float* xb = x + (long)b * img * 64;
  const float* wb = wm + (long)b * img * 64;
  if (blockIdx.x < AAS_F) {
    const int h = blockIdx.x;
    const long base = ((long)(h + 1) * wp + 1) * 64 + c;
    float mx = -INFINITY;
    for (int w = 0; w < wd; ++w) mx = fmaxf(mx, wb[base + (long)w * 64]);
    float den = 0.f, num = 0.f;
    for (int w = 0; w < wd; ++w) {
      const float e = expf(wb[base + (long)w * 64] - mx);
      den += e;
      num = fmaf(xb[base + (long)w * 64], e, num);
    }
    eS[((long)b * AAS_F + h) * 64 + c] = num / den + pos_S[h * 64 + c];
  } else {
    const int w = blockIdx.x - AAS_F;
    const long base = ((long)wp + w + 1) * 64 + c;
    const long st = (long)wp * 64;
    float mx = -INFINITY;
    for (int h = 0; h < AAS_F; ++h) mx = fmaxf(mx, wb[base + h * st]);
    float den = 0.f, num = 0.f;
    for (int h = 0; h < AAS_F; ++h) {
      const float e = expf(wb[base + h * st] - mx);
      den += e;
      num = fmaf(xb[base + h * st], e, num);
    }
    eT[((long)b * wd + w) * 64 + c] = num / den;
  }
}

// Several independent small problems of one shape class in ONE launch (blockIdx.z picks the problem): the graph stage is
// a chain of launches a few microseconds long, and its two HS-GAL branches, the spectral / temporal graphs and the two
// node types of a layer are independent of each other -- 21 launches per forward become 8.
struct RowlinArgs {
  const float* x; long ldx; int rows, K; const float *W, *bias; int N; float* y; long ldy; int rpb, o_batch_rows, o_row_off;
};
struct RowlinMulti { RowlinArgs q[4]; };
// y[r][o] = b[o] + W[o] . x[r]   (rows of <= 64 features; wave per row, lane per output)
__global__ void rowlin_kernel(RowlinMulti mm) {
  const RowlinArgs& q = mm.q[blockIdx.z];
  const float* __restrict__ x = q.x;
  const float* __restrict__ W = q.W;
  const float* __restrict__ bias = q.bias;
  float* __restrict__ y = q.y;
  const long ldx = q.ldx, ldy = q.ldy;
  const int rows = q.rows, K = q.K, N = q.N, rpb = q.rpb, o_batch_rows = q.o_batch_rows, o_row_off = q.o_row_off;
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows || lane >= N) return;
  const float* xr = x + (long)r * ldx;
  const float* wr = W + (long)lane * K;
  float a = bias[lane];
  for (int k = 0; k < K; ++k) a = fmaf(wr[k], xr[k], a);
  const long orow = (long)(r / rpb) * o_batch_rows + (r % rpb) + o_row_off;
  y[orow * ldy + lane] = a;
}

// ===================================================================================
// graph attention (GraphAttentionLayer and the node/master parts of HtrgGraphAttention
// Layer, models/aasist_modules.py:17-110,112-294).  Grid (N [+1], B): block i updates
// node i; for the heterogeneous layer block N updates the master node.
//   att[i][j] = softmax_j( tanh(W_att (x_i * x_j) + b) . v_blk(i,j) / temp )
//   out_i = SELU(BN(W1 (sum_j att[i][j] x_j) + b1 + W2 x_i + b2))
// The (N,N,D) pairwise tensor is never materialised: thread o keeps row o of W_att
// pre-multiplied by x_i in registers and streams x_j from LDS.
// ===================================================================================
struct GatArgs {
  const float* x;  // (B, N, DIN) node features (already type-projected for the htrg layer)
  int N, n1;       // n1 = nodes of type 1 (== N for the homogeneous layer)
  const float *att_w, *att_b;       // [DOUT][DIN], [DOUT]
  const float *v11, *v22, *v12;     // [DOUT] each (homogeneous: all the same)
  const float *w1, *b1, *w2, *b2;   // proj_with_att / proj_without_att
  const float *bn_scale, *bn_shift;
  float temp;
  float* y1;  // (B, n1, DOUT)
  float* y2;  // (B, N-n1, DOUT)
  // master (htrg only; master == nullptr disables)
  const float* master;  // (B or 1, DIN)
  long master_bstride;  // 0 when the parameter is shared by the batch
  const float *attM_w, *attM_b, *vM, *w1M, *b1M, *w2M, *b2M;
  float* master_out;  // (B, DOUT)
};

struct GatMulti { GatArgs a[2]; };
template <int DIN, int DOUT>
__global__ __launch_bounds__(256) void gat_kernel(GatMulti pp) {
  constexpr int JPW = 64 / DOUT;  // nodes handled at once by one wave
  // dynamic LDS, sized by the launcher for the larger graph: node features, attention row, aggregate
  extern __shared__ __attribute__((aligned(16))) float gat_lds[];
  const GatArgs& p = pp.a[blockIdx.z];
  const int b = blockIdx.y, i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = p.N;
  if (i > N || (i == N && !p.master)) return;  // the grid covers the larger of the two graphs (+ its master node)
  float* xs = gat_lds;                     // [N][DIN]
  float* agg = xs + (long)N * DIN;         // [64]
  float* att = agg + 64;                   // [N]
  const bool is_master = i == N;
  const float* xb = p.x + (long)b * N * DIN;
  for (int idx = tid; idx < N * DIN / 4; idx += 256) *(f32x4*)(xs + idx * 4) = *(const f32x4*)(xb + idx * 4);
  __syncthreads();
  const int o = lane % DOUT, jsub = lane / DOUT;
  // centre vector: x_i for a node, the master vector for the master update
  const float* ctr = is_master ? p.master + (long)b * p.master_bstride : xs + i * DIN;
  const float* aw = is_master ? p.attM_w : p.att_w;
  float wi[DIN];
#pragma unroll
  for (int d = 0; d < DIN; ++d) wi[d] = aw[o * DIN + d] * ctr[d];
  const float ab = is_master ? p.attM_b[o] : p.att_b[o];
  for (int j0 = wave * JPW; j0 < N; j0 += 4 * JPW) {
    const int j = j0 + jsub;
    const int jc = j < N ? j : N - 1;
    float h = ab;
#pragma unroll
    for (int d = 0; d < DIN; d += 4) {
      const f32x4 xv = *(const f32x4*)(xs + jc * DIN + d);
      h = fmaf(wi[d], xv[0], h);
      h = fmaf(wi[d + 1], xv[1], h);
      h = fmaf(wi[d + 2], xv[2], h);
      h = fmaf(wi[d + 3], xv[3], h);
    }
    const float* vv = is_master ? p.vM : ((i < p.n1) == (jc < p.n1) ? (i < p.n1 ? p.v11 : p.v22) : p.v12);
    float t = tanhf(h) * vv[o];
#pragma unroll
    for (int off = DOUT / 2; off > 0; off >>= 1) t += __shfl_xor(t, off, 64);
    if (o == 0 && j < N) att[j] = t / p.temp;
  }
  __syncthreads();
  if (wave == 0) {  // softmax over j: lane l takes nodes l, l + 64, ...
    float mx = -INFINITY;
    for (int j = lane; j < N; j += 64) mx = fmaxf(mx, att[j]);
    mx = wave_max(mx);
    float part = 0.f;
    for (int j = lane; j < N; j += 64) {
      const float e = expf(att[j] - mx);
      att[j] = e;
      part += e;
    }
    const float den = wave_sum(part);
    for (int j = lane; j < N; j += 64) att[j] = att[j] / den;
  }
  __syncthreads();
  if (tid < DIN) {
    float a = 0.f;
    for (int j = 0; j < N; ++j) a = fmaf(att[j], xs[j * DIN + tid], a);
    agg[tid] = a;
  }
  __syncthreads();
  if (tid < DOUT) {
    const float* W1 = is_master ? p.w1M : p.w1;
    const float* W2 = is_master ? p.w2M : p.w2;
    float a = is_master ? p.b1M[tid] : p.b1[tid];
    float c = is_master ? p.b2M[tid] : p.b2[tid];
    for (int d = 0; d < DIN; ++d) {
      a = fmaf(W1[tid * DIN + d], agg[d], a);
      c = fmaf(W2[tid * DIN + d], ctr[d], c);
    }
    const float v = a + c;
    if (is_master) {
      p.master_out[(long)b * DOUT + tid] = v;
    } else {
      const float y = selu(fmaf(v, p.bn_scale[tid], p.bn_shift[tid]));
      if (i < p.n1)
        p.y1[((long)b * p.n1 + i) * DOUT + tid] = y;
      else
        p.y2[((long)b * (N - p.n1) + (i - p.n1)) * DOUT + tid] = y;
    }
  }
}

// one or two graphs of the same layer dims in one launch (a1 may be null)
static const char* launch_gat(const GatArgs& a, int B, int din, int dout, hipStream_t s, const GatArgs* a1 = nullptr) {
  // one workgroup per node keeps the whole graph's features in LDS: 4-s clips have <= 66 nodes (17 KB); the
  // 160 KB of a CU hold AAS_MAX_NODES = 629 nodes of 64 features ((65 N + 72) floats <= 40 960) = clips of about
  // 37 s (test_duration_sec is a free config value); aasist_forward refuses longer clips before anything is launched
  const int nmax = a1 && a1->N > a.N ? a1->N : a.N;
  const int lds = (int)(((long)nmax * din + 64 + nmax + 8) * sizeof(float));
  if (a.N < 1 || (a1 && a1->N < 1) || lds > 160 * 1024) return "aasist: graph has too many nodes for the LDS slab (clip longer than ~37 s)";
  GatMulti mm;
  mm.a[0] = a;
  mm.a[1] = a1 ? *a1 : a;
  dim3 grid(nmax + ((a.master || (a1 && a1->master)) ? 1 : 0), B, a1 ? 2 : 1);
  hipError_t e = hipSuccess;
  static LdsLimit lim[3];
#define AFX_GAT(IDX, DI, DO)                                                                                          \
  do {                                                                                                                \
    if (lds > 48 * 1024) e = lim[IDX].ensure((const void*)gat_kernel<DI, DO>, lds);                                   \
    if (e == hipSuccess) hipLaunchKernelGGL((gat_kernel<DI, DO>), grid, dim3(256), lds, s, mm);                       \
  } while (0)
  if (din == 64 && dout == 64)
    AFX_GAT(0, 64, 64);
  else if (din == 64 && dout == 32)
    AFX_GAT(1, 64, 32);
  else if (din == 32 && dout == 32)
    AFX_GAT(2, 32, 32);
  else
    return "aasist: unsupported graph layer dims";
#undef AFX_GAT
  if (e == hipSuccess) e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

// GraphPool (models/aasist_modules.py:296-338): s = sigmoid(w.h + b); keep the top
// max(int(N*k),1) nodes in DESCENDING score order; out = h * s.  One block per utterance.
struct PoolArgs { const float* h; int N, D, keep; const float *w, *bias; float* out; };
struct PoolMulti { PoolArgs q[4]; };
__global__ void graph_pool_kernel(PoolMulti mm) {
  const PoolArgs& a = mm.q[blockIdx.z];
  const float* __restrict__ h = a.h;
  const float* __restrict__ w = a.w;
  const float* __restrict__ bias = a.bias;
  float* __restrict__ out = a.out;
  const int N = a.N, D = a.D, keep = a.keep;
  extern __shared__ float sc[];  // [N]; one thread per node (block = the largest N rounded up to a wave)
  const int b = blockIdx.x, j = threadIdx.x;
  const float* hb = h + (long)b * N * D;
  if (j < N) {
    float a = bias[0];
    for (int d = 0; d < D; ++d) a = fmaf(hb[j * D + d], w[d], a);
    sc[j] = sigmoid_acc(a);
  }
  __syncthreads();
  if (j < N) {
    const float s = sc[j];
    int rank = 0;
    for (int q = 0; q < N; ++q) rank += (sc[q] > s) || (sc[q] == s && q < j);
    if (rank < keep)
      for (int d = 0; d < D; ++d) out[((long)b * keep + rank) * D + d] = hb[j * D + d] * s;
  }
}

static void launch_pools(const PoolArgs* q, int n, int B, hipStream_t s) {
  PoolMulti mm;
  int nmax = 1;
  for (int i = 0; i < 4; ++i) {
    mm.q[i] = q[i < n ? i : 0];
    if (i < n && q[i].N > nmax) nmax = q[i].N;
  }
  hipLaunchKernelGGL(graph_pool_kernel, dim3(B, 1, n), dim3((nmax + 63) & ~63), (nmax + 8) * sizeof(float), s, mm);
}
static void launch_rowlins(const RowlinArgs* q, int n, hipStream_t s) {
  RowlinMulti mm;
  int rmax = 1;
  for (int i = 0; i < 4; ++i) {
    mm.q[i] = q[i < n ? i : 0];
    if (i < n && q[i].rows > rmax) rmax = q[i].rows;
  }
  hipLaunchKernelGGL(rowlin_kernel, dim3((rmax + 3) / 4, 1, n), dim3(256), 0, s, mm);
}

// models/xlsr_aasist.py:137-175: residual adds (incl. the literal "+ 1", Q1), branch max,
// readout [max|T|, mean T, max|S|, mean S, master] and the 160 -> 2 output layer.
__global__ void readout_kernel(const float* T1, const float* Ta1, const float* S1, const float* m1, const float* ma1,
                               const float* T2, const float* Ta2, const float* S2, const float* Sa2, const float* m2,
                               const float* ma2, int nT, int nS, const float* __restrict__ ow,
                               const float* __restrict__ ob, float* __restrict__ hidden, float* __restrict__ logits,
                               int* __restrict__ nonfinite) {
  __shared__ float hid[160];
  const int b = blockIdx.x, d = threadIdx.x;  // 32 threads
  float tmax = 0.f, tsum = 0.f;
  for (int n = 0; n < nT; ++n) {
    const long o = ((long)b * nT + n) * 32 + d;
    const float v = fmaxf(T1[o] + Ta1[o], T2[o] + Ta2[o]);
    tmax = n == 0 ? fabsf(v) : fmaxf(tmax, fabsf(v));
    tsum += v;
  }
  float smax = 0.f, ssum = 0.f;
  for (int n = 0; n < nS; ++n) {
    const long o = ((long)b * nS + n) * 32 + d;
    const float v = fmaxf(S1[o] + 1.0f, S2[o] + Sa2[o]);  // Q1: branch 1 adds the constant 1
    smax = n == 0 ? fabsf(v) : fmaxf(smax, fabsf(v));
    ssum += v;
  }
  const long mo = (long)b * 32 + d;
  hid[d] = tmax;
  hid[32 + d] = tsum / (float)nT;
  hid[64 + d] = smax;
  hid[96 + d] = ssum / (float)nS;
  hid[128 + d] = fmaxf(m1[mo] + ma1[mo], m2[mo] + ma2[mo]);
  __syncthreads();
  for (int k = d; k < 160; k += 32) hidden[(long)b * 160 + k] = hid[k];
  if (d < 2) {
    float a = ob[d];
    for (int k = 0; k < 160; ++k) a = fmaf(ow[d * 160 + k], hid[k], a);
    logits[b * 2 + d] = a;
    if (nonfinite && !(fabsf(a) <= 3.0e38f)) atomicAdd(nonfinite, 1);  // overflow guard (NaN fails the compare too)
  }
}

// ===================================================================================
// host side
// ===================================================================================
static const float kEps = 1e-5f;

const char* aasist_finalize(AasistWeights& w, const GetF& get, const Alloc& alloc, hipStream_t s) {
  static thread_local std::string err;
  auto need = [&](const std::string& k) -> const float* {
    const float* p = get(k);
    if (!p && err.empty()) err = "missing weight '" + k + "'";
    return p;
  };
  err.clear();
  auto fold = [&](const std::string& pre, int n, float** sc, float** sh) {
    const float *g = need(pre + "weight"), *b = need(pre + "bias"), *m = need(pre + "running_mean"),
                *v = need(pre + "running_var");
    *sc = (float*)alloc((size_t)n * 4);
    *sh = (float*)alloc((size_t)n * 4);
    if (g && b && m && v && *sc && *sh)
      hipLaunchKernelGGL(bn_fold2_kernel, dim3((n + 63) / 64), dim3(64), 0, s, g, b, m, v, kEps, n, *sc, *sh);
  };
  auto pack = [&](const std::string& k, int cout, int cin, int kh, int kw) -> float* {
    const float* src = need(k);
    float* dst = (float*)alloc((size_t)cout * cin * kh * kw * 4);
    if (src && dst) hipLaunchKernelGGL(pack_conv2d_kernel, dim3(64), dim3(256), 0, s, src, cout, cin, kh, kw, dst);
    return dst;
  };
  // split-precision copies (hi, lo) of a packed fp32 weight for f32s_gemm_kernel; null pair in exact mode
  auto split = [&](const float* src, size_t n, AasistWeights::Split* out) {
    out->hi = out->lo = nullptr;
    if (!w.split || !src) return;
    out->hi = (_Float16*)alloc(n * 2);
    out->lo = (_Float16*)alloc(n * 2);
    if (out->hi && out->lo)
      hipLaunchKernelGGL(split_f16_kernel, dim3(64), dim3(256), 0, s, src, (long)n, out->hi, out->lo);
  };
  w.LLw = need("LL.weight");
  w.LLb = need("LL.bias");
  split(w.LLw, (size_t)128 * 1024, &w.LLs);
  static const int filt[6][2] = {{1, 32}, {32, 32}, {32, 64}, {64, 64}, {64, 64}, {64, 64}};
  for (int i = 0; i < 6; ++i) {
    AasistWeights::Block& B = w.blk[i];
    const std::string p = "encoder." + std::to_string(i) + ".0.";
    B.cin = filt[i][0];
    B.cout = filt[i][1];
    B.w1 = pack(p + "conv1.weight", B.cout, B.cin, 2, 3);
    B.b1 = need(p + "conv1.bias");
    B.w2 = pack(p + "conv2.weight", B.cout, B.cout, 2, 3);
    B.b2 = need(p + "conv2.bias");
    if (B.cin > 1) split(B.w1, (size_t)B.cout * B.cin * 6, &B.s1);
    split(B.w2, (size_t)B.cout * B.cout * 6, &B.s2);
    fold(p + "bn2.", B.cout, &B.bn2_scale, &B.bn2_shift);
    B.wd = nullptr;
    B.bd = nullptr;
    if (B.cin != B.cout) {
      B.wd = pack(p + "conv_downsample.weight", B.cout, B.cin, 1, 3);
      B.bd = need(p + "conv_downsample.bias");
      if (B.cin > 1) split(B.wd, (size_t)B.cout * B.cin * 3, &B.sd);
    }
  }
  fold("first_bn1.", 64, &w.bn1_scale, &w.bn1_shift);
  w.att_w0 = pack("attention.0.weight", 128, 64, 1, 1);
  w.att_b0 = need("attention.0.bias");
  split(w.att_w0, (size_t)128 * 64, &w.att_s0);
  fold("attention.2.", 128, &w.att_bn_scale, &w.att_bn_shift);
  w.att_w3 = pack("attention.3.weight", 64, 128, 1, 1);
  w.att_b3 = need("attention.3.bias");
  split(w.att_w3, (size_t)64 * 128, &w.att_s3);
  w.pos_S = need("pos_S");
  w.master1 = need("master1");
  w.master2 = need("master2");
  auto gat = [&](AasistWeights::Gat& g, const std::string& p) {
    g.att_w = need(p + "att_proj.weight");
    g.att_b = need(p + "att_proj.bias");
    g.att_vec = need(p + "att_weight");
    g.w1 = need(p + "proj_with_att.weight");
    g.b1 = need(p + "proj_with_att.bias");
    g.w2 = need(p + "proj_without_att.weight");
    g.b2 = need(p + "proj_without_att.bias");
    fold(p + "bn.", 64, &g.bn_scale, &g.bn_shift);
  };
  gat(w.gatS, "GAT_layer_S.");
  gat(w.gatT, "GAT_layer_T.");
  auto hgat = [&](AasistWeights::HGat& g, const std::string& p, int din, int dout) {
    g.din = din;
    g.dout = dout;
    g.t1w = need(p + "proj_type1.weight"); g.t1b = need(p + "proj_type1.bias");
    g.t2w = need(p + "proj_type2.weight"); g.t2b = need(p + "proj_type2.bias");
    g.att_w = need(p + "att_proj.weight"); g.att_b = need(p + "att_proj.bias");
    g.attM_w = need(p + "att_projM.weight"); g.attM_b = need(p + "att_projM.bias");
    g.v11 = need(p + "att_weight11"); g.v22 = need(p + "att_weight22");
    g.v12 = need(p + "att_weight12"); g.vM = need(p + "att_weightM");
    g.w1 = need(p + "proj_with_att.weight"); g.b1 = need(p + "proj_with_att.bias");
    g.w2 = need(p + "proj_without_att.weight"); g.b2 = need(p + "proj_without_att.bias");
    g.w1M = need(p + "proj_with_attM.weight"); g.b1M = need(p + "proj_with_attM.bias");
    g.w2M = need(p + "proj_without_attM.weight"); g.b2M = need(p + "proj_without_attM.bias");
    fold(p + "bn.", dout, &g.bn_scale, &g.bn_shift);
  };
  hgat(w.h11, "HtrgGAT_layer_ST11.", 64, 32);
  hgat(w.h12, "HtrgGAT_layer_ST12.", 32, 32);
  hgat(w.h21, "HtrgGAT_layer_ST21.", 64, 32);
  hgat(w.h22, "HtrgGAT_layer_ST22.", 32, 32);
  auto pool = [&](AasistWeights::Pool& q, const std::string& p) {
    q.w = need(p + "proj.weight");
    q.b = need(p + "proj.bias");
  };
  pool(w.pS, "pool_S."); pool(w.pT, "pool_T.");
  pool(w.phS1, "pool_hS1."); pool(w.phT1, "pool_hT1.");
  pool(w.phS2, "pool_hS2."); pool(w.phT2, "pool_hT2.");
  w.out_w = need("out_layer.weight");
  w.out_b = need("out_layer.bias");
  // BatchNorm2d(1) of the front: scalars to the host (one-off sync)
  const float *g0 = need("first_bn.weight"), *b0 = need("first_bn.bias"), *m0 = need("first_bn.running_mean"),
              *v0 = need("first_bn.running_var");
  if (!err.empty()) return err.c_str();
  if (hipStreamSynchronize(s) != hipSuccess) return "aasist: stream sync failed";
  float hw, hb, hm, hv;
  if (hipMemcpy(&hw, g0, 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(&hb, b0, 4, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(&hm, m0, 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(&hv, v0, 4, hipMemcpyDeviceToHost) != hipSuccess)
    return "aasist: reading first_bn failed";
  w.bn0_scale = hw / sqrtf(hv + kEps);
  w.bn0_shift = hb - hm * w.bn0_scale;
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hipGetErrorString(e);
  w.ready = true;
  return nullptr;
}

static void dims(int T, int* wd, int* wp, int* img) {
  *wd = T / 3;
  *wp = *wd + 2;
  *img = AAS_HP * *wp;
}

void aasist_carve(int B, int T, const Alloc& take, AasistWs* ws) {
  int wd, wp, img;
  dims(T, &wd, &wp, &img);
  const size_t pix = (size_t)B * img + 3 * (size_t)wp + 16;  // + slack for the shifted reads / writes
  ws->ll = (float*)take((size_t)B * T * 128 * 4);
  ws->imgA = (float*)take(pix * 64 * 4);
  ws->imgB = (float*)take(pix * 64 * 4);
  ws->imgC = (float*)take(pix * 64 * 4);
  ws->wmap1 = (float*)take(pix * 128 * 4);
  ws->wmap2 = (float*)take(pix * 64 * 4);
  ws->eS = (float*)take((size_t)B * AAS_F * 64 * 4);
  ws->eT = (float*)take((size_t)B * (wd > 0 ? wd : 1) * 64 * 4);
  ws->gS = (float*)take((size_t)B * AAS_F * 64 * 4);
  ws->gT = (float*)take((size_t)B * (wd > 0 ? wd : 1) * 64 * 4);
  ws->oS = (float*)take((size_t)B * AAS_F * 64 * 4);
  ws->oT = (float*)take((size_t)B * (wd > 0 ? wd : 1) * 64 * 4);
  ws->br = (float*)take(((size_t)B * 2 * 3 * (AAS_F + (wd > 0 ? wd : 1) + 16) * 64 + 2 * 10 * 64) * 4);
  ws->hidden = (float*)take((size_t)B * 160 * 4);
}

#define AOK(expr)                  \
  do {                             \
    const char* m_ = (expr);       \
    if (m_) return m_;             \
  } while (0)
#define HOK(expr)                                          \
  do {                                                     \
    hipError_t e_ = (expr);                                \
    if (e_ != hipSuccess) return hipGetErrorString(e_);    \
  } while (0)

// diagnostic knob (tools/diag_two_stream_which.py): > 0 = the back-end returns after that many of its stages (logits are then
// whatever the buffer held) -- which stage's kernels disturb a trunk running beside them on another stream
static int g_aas_stop = 0;
void aasist_set_stop(int v) { g_aas_stop = v; }
#define AAS_STAGE()                                   \
  do {                                                \
    if (g_aas_stop > 0 && ++stage_ == g_aas_stop) return nullptr; \
  } while (0)

const char* aasist_forward(const AasistWeights& w, const float* feats, int B, int T, AasistWs& ws, float* logits,
                           hipStream_t s, int* nonfinite) {
  if (!w.ready) return "aasist: weights not finalized";
  int stage_ = 0;
  int wd, wp, img;
  dims(T, &wd, &wp, &img);
  if (wd < 2) return "aasist: clip too short (need at least 6 SSL frames)";
  if (wd > AAS_MAX_NODES) return "aasist: clip too long for the graph kernels (about 37 s: T <= 1889 frames)";
  const int M = B * img;
  // test hook: nothing but this null check when taps are off; images are handed over whole in their padded layout
  // ((M + wp + 1) pixel rows), so that their borders can be checked
#define ATAP(nm, ptr, cnt)                                                                              \
  do {                                                                                                  \
    if (ws.tap && ws.tap(ws.tap_ctx, std::string(nm).c_str(), (ptr), (size_t)(cnt))) return "aasist: tap failed"; \
  } while (0)
  const size_t ipix = (size_t)M + wp + 1;
  // ---- LL: (B*T,1024) x [128][1024] on the fp32 matrix cores ------------------------
  {
    F32GemmArgs g;
    memset(&g, 0, sizeof g);
    g.A = feats; g.lda = 1024; g.nch = 1; g.kc = 1024; g.W = w.LLw; g.Wh = w.LLs.hi; g.Wl = w.LLs.lo; g.M = B * T; g.N = 128;
    g.bias = w.LLb; g.out = ws.ll; g.ldo = 128;
    AOK(launch_f32_gemm(g, s));
  }
  ATAP("aa.ll", ws.ll, (size_t)B * T * 128);
  AAS_STAGE();  // 1: LL
  // ---- max-pool + BN + SELU into a 1-channel padded image ---------------------------
  float *X = ws.imgA, *Y = ws.imgB, *D = ws.imgC;
  // Only what no kernel writes has to be zeroed: every conv stores ALL virtual pixels at rows [wp+1, M+wp+1) (zeros
  // where they fall in the padding -- that re-creates the border), so of each image just the first padded row + 1
  // pixel; rows past M+wp+1 are read by invalid (masked-by-assignment) outputs only.  (Round 1 cleared 3 x 12.8 MB
  // per forward here.)
  const int head = (wp + 1) * 64;  // first padded row + 1 pixel, 64 channels (floats)
  float* x1 = ws.wmap2;  // 1-channel image borrowed from a later buffer
  hipLaunchKernelGGL(pool_bn_selu_kernel, dim3((img + 255) / 256, B + 1), dim3(256), 0, s, ws.ll, T, wd, wp, img,
                     w.bn0_scale, w.bn0_shift, x1, B, 3 * wp + 16, ws.imgA, ws.imgB, ws.imgC, head);
  ATAP("aa.x1", x1, (size_t)M + 3 * wp + 16);
  AAS_STAGE();  // 2: pooling
  // ---- residual encoder ----------------------------------------------------------------
  {  // block 0 (Cin = 1): conv1+bn2+selu -> Y, downsample -> D, conv2(Y) + D -> X
    const AasistWeights::Block& K = w.blk[0];
    const long n = (long)M * K.cout;
    hipLaunchKernelGGL(first_block_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x1, M, img, wp, wd, K.w1,
                       K.b1, K.bn2_scale, K.bn2_shift, K.wd, K.bd, Y, D, K.cout, AAS_F);
    ATAP("aa.b0.y", Y, ipix * K.cout);
    ATAP("aa.b0.d", D, ipix * K.cout);
    F32GemmArgs g;
    memset(&g, 0, sizeof g);
    g.A = Y + (long)wp * K.cout; g.lda = K.cout; g.nch = 2; g.kc = 3 * K.cout; g.chunk_stride = (long)wp * K.cout;
    g.W = K.w2; g.Wh = K.s2.hi; g.Wl = K.s2.lo; g.M = M; g.N = K.cout; g.bias = K.b2; g.resid = D;
    g.img = img; g.wp = wp; g.hout = AAS_F; g.wd = wd; g.out = X; g.ldo = K.cout; g.o_off = wp + 1;
    AOK(launch_f32_gemm(g, s));
    ATAP("aa.b0", X, ipix * K.cout);
  }
  AAS_STAGE();  // 3: residual block 0
  for (int i = 1; i < 6; ++i) {
    const AasistWeights::Block& K = w.blk[i];
    F32GemmArgs g;
    memset(&g, 0, sizeof g);  // conv1 (pad (1,1)) on X -> bn2 -> selu -> Y, 43 rows
    g.A = X; g.lda = K.cin; g.nch = 2; g.kc = 3 * K.cin; g.chunk_stride = (long)wp * K.cin;
    g.W = K.w1; g.Wh = K.s1.hi; g.Wl = K.s1.lo; g.M = M; g.N = K.cout; g.bias = K.b1; g.bn_scale = K.bn2_scale; g.bn_shift = K.bn2_shift; g.post = 1;
    g.img = img; g.wp = wp; g.hout = AAS_F + 1; g.wd = wd; g.out = Y; g.ldo = K.cout; g.o_off = wp + 1;
    AOK(launch_f32_gemm(g, s));
    const float* resid = X;
    if (K.wd) {  // (1,3) downsample conv of X -> D
      memset(&g, 0, sizeof g);
      g.A = X + (long)wp * K.cin; g.lda = K.cin; g.nch = 1; g.kc = 3 * K.cin; g.W = K.wd; g.Wh = K.sd.hi; g.Wl = K.sd.lo; g.M = M; g.N = K.cout;
      g.bias = K.bd; g.img = img; g.wp = wp; g.hout = AAS_F; g.wd = wd; g.out = D; g.ldo = K.cout; g.o_off = wp + 1;
      AOK(launch_f32_gemm(g, s));
      resid = D;
      // X, Y and D switch to cout channels per pixel: the first padded row + 1 pixel of each is never touched by the
      // shifted stores (conv1 -> Y and the downsample -> D above wrote from pixel wp+1 on) and still holds cin-channel
      // data; X's may go only now that both convs have read it
      if (K.cin != K.cout) hipLaunchKernelGGL(zero3_kernel, dim3((head + 255) / 256), dim3(256), 0, s, X, Y, D, head);
    }
    if (ws.tap) {  // (after the heads are cleared: what conv2 reads)
      const std::string nm = "aa.b" + std::to_string(i);
      ATAP(nm + ".y", Y, ipix * K.cout);
      if (K.wd) ATAP(nm + ".d", D, ipix * K.cout);
    }
    // conv2 (pad (0,1)) on Y + residual, written over X (each element is read, as the
    // residual, by the same thread that then overwrites it)
    memset(&g, 0, sizeof g);
    g.A = Y + (long)wp * K.cout; g.lda = K.cout; g.nch = 2; g.kc = 3 * K.cout; g.chunk_stride = (long)wp * K.cout;
    g.W = K.w2; g.Wh = K.s2.hi; g.Wl = K.s2.lo; g.M = M; g.N = K.cout; g.bias = K.b2; g.resid = resid;
    if (i == 5) {  // first_bn1 + SELU close the encoder (models/xlsr_aasist.py:100-101)
      g.bn_scale = w.bn1_scale; g.bn_shift = w.bn1_shift; g.post = 1;
    }
    g.img = img; g.wp = wp; g.hout = AAS_F; g.wd = wd; g.out = X; g.ldo = K.cout; g.o_off = wp + 1;
    AOK(launch_f32_gemm(g, s));
    if (ws.tap) ATAP("aa.b" + std::to_string(i), X, ipix * K.cout);
    AAS_STAGE();  // 4..8: residual blocks 1..5
  }
  // ---- attention maps: 1x1 convs over the padded image --------------------------------
  {
    F32GemmArgs g;
    memset(&g, 0, sizeof g);
    g.A = X; g.lda = 64; g.nch = 1; g.kc = 64; g.W = w.att_w0; g.Wh = w.att_s0.hi; g.Wl = w.att_s0.lo; g.M = M; g.N = 128; g.bias = w.att_b0;
    g.bn_scale = w.att_bn_scale; g.bn_shift = w.att_bn_shift; g.post = 2; g.out = ws.wmap1; g.ldo = 128;
    AOK(launch_f32_gemm(g, s));
    ATAP("aa.w1", ws.wmap1, (size_t)M * 128);
    memset(&g, 0, sizeof g);
    g.A = ws.wmap1; g.lda = 128; g.nch = 1; g.kc = 128; g.W = w.att_w3; g.Wh = w.att_s3.hi; g.Wl = w.att_s3.lo; g.M = M; g.N = 64; g.bias = w.att_b3;
    g.out = ws.wmap2; g.ldo = 64;
    AOK(launch_f32_gemm(g, s));
    ATAP("aa.w2", ws.wmap2, (size_t)M * 64);
  }
  hipLaunchKernelGGL(att_pool_kernel, dim3(AAS_F + wd, B), dim3(64), 0, s, X, ws.wmap2, img, wp, wd, w.pos_S, ws.eS,
                     ws.eT);
  AAS_STAGE();  // 9: attention maps + pooling
  // ---- graph layers ---------------------------------------------------------------------
  const int nS = AAS_F / 2, nT = wd / 2 > 0 ? wd / 2 : 1;        // after pool_S / pool_T
  const int nS1 = nS / 2 > 0 ? nS / 2 : 1, nT1 = nT / 2 > 0 ? nT / 2 : 1;  // after pool_h*
  auto gat_args = [&](const AasistWeights::Gat& G, const float* x, int N, float* y) {
    GatArgs a;
    memset(&a, 0, sizeof a);
    a.x = x; a.N = N; a.n1 = N; a.att_w = G.att_w; a.att_b = G.att_b; a.v11 = a.v22 = a.v12 = G.att_vec;
    a.w1 = G.w1; a.b1 = G.b1; a.w2 = G.w2; a.b2 = G.b2; a.bn_scale = G.bn_scale; a.bn_shift = G.bn_shift;
    a.temp = 2.0f; a.y1 = y; a.y2 = y;
    return a;
  };
  auto pool_args = [&](const AasistWeights::Pool& P, const float* h, int N, int Dm, int keep, float* out) {
    return PoolArgs{h, N, Dm, keep, P.w, P.b, out};
  };
  {  // the spectral and the temporal graph in one launch each: GAT, then GraphPool
    const GatArgs gS = gat_args(w.gatS, ws.eS, AAS_F, ws.gS), gT = gat_args(w.gatT, ws.eT, wd, ws.gT);
    AOK(launch_gat(gS, B, 64, 64, s, &gT));
    const PoolArgs pp[2] = {pool_args(w.pS, ws.gS, AAS_F, 64, nS, ws.oS), pool_args(w.pT, ws.gT, wd, 64, nT, ws.oT)};
    launch_pools(pp, 2, B, s);
  }
  AAS_STAGE();  // 10: GAT + GraphPool of both graphs
  // branch scratch carve
  float* p = ws.br;
  auto take = [&](size_t n) { float* r = p; p += (n + 63) / 64 * 64; return r; };
  struct Branch { float *xp, *T1, *S1, *m1, *T1p, *S1p, *xp2, *Ta, *Sa, *ma; } br[2];
  for (int k = 0; k < 2; ++k) {
    br[k].xp = take((size_t)B * (nT + nS) * 64);
    br[k].T1 = take((size_t)B * nT * 32);
    br[k].S1 = take((size_t)B * nS * 32);
    br[k].m1 = take((size_t)B * 32);
    br[k].T1p = take((size_t)B * nT1 * 32);
    br[k].S1p = take((size_t)B * nS1 * 32);
    br[k].xp2 = take((size_t)B * (nT1 + nS1) * 32);
    br[k].Ta = take((size_t)B * nT1 * 32);
    br[k].Sa = take((size_t)B * nS1 * 32);
    br[k].ma = take((size_t)B * 32);
  }
  // one heterogeneous layer of BOTH branches: type projections (4 problems, one launch), then the two graphs (one launch)
  auto hgat_args = [&](const AasistWeights::HGat& G, int n1, int n2, float* xp, const float* master, long mstride, float* y1,
                       float* y2, float* mout) {
    GatArgs a;
    memset(&a, 0, sizeof a);
    a.x = xp; a.N = n1 + n2; a.n1 = n1; a.att_w = G.att_w; a.att_b = G.att_b; a.v11 = G.v11; a.v22 = G.v22; a.v12 = G.v12;
    a.w1 = G.w1; a.b1 = G.b1; a.w2 = G.w2; a.b2 = G.b2; a.bn_scale = G.bn_scale; a.bn_shift = G.bn_shift;
    a.temp = 100.0f; a.y1 = y1; a.y2 = y2;
    a.master = master; a.master_bstride = mstride; a.attM_w = G.attM_w; a.attM_b = G.attM_b; a.vM = G.vM;
    a.w1M = G.w1M; a.b1M = G.b1M; a.w2M = G.w2M; a.b2M = G.b2M; a.master_out = mout;
    return a;
  };
  auto proj_args = [&](const AasistWeights::HGat& G, bool second, const float* x, int n, int N, int off, float* xp) {
    return RowlinArgs{x, (long)G.din, B * n, G.din, second ? G.t2w : G.t1w, second ? G.t2b : G.t1b, G.din, xp, (long)G.din, n, N, off};
  };
  const AasistWeights::HGat* H1[2] = {&w.h11, &w.h21};
  const AasistWeights::HGat* H2[2] = {&w.h12, &w.h22};
  const AasistWeights::Pool* PS[2] = {&w.phS1, &w.phS2};
  const AasistWeights::Pool* PT[2] = {&w.phT1, &w.phT2};
  const float* M0[2] = {w.master1, w.master2};
  {
    // layer 1: x1 = temporal nodes, x2 = spectral nodes (models/xlsr_aasist.py:129-130); the raw (1,1,64) parameter is
    // the master of the first layer (Q3)
    RowlinArgs pr[4];
    GatArgs ga[2];
    for (int k = 0; k < 2; ++k) {
      pr[2 * k] = proj_args(*H1[k], false, ws.oT, nT, nT + nS, 0, br[k].xp);
      pr[2 * k + 1] = proj_args(*H1[k], true, ws.oS, nS, nT + nS, nT, br[k].xp);
      ga[k] = hgat_args(*H1[k], nT, nS, br[k].xp, M0[k], 0, br[k].T1, br[k].S1, br[k].m1);
    }
    launch_rowlins(pr, 4, s);
    AOK(launch_gat(ga[0], B, H1[0]->din, H1[0]->dout, s, &ga[1]));
    PoolArgs pp[4];
    for (int k = 0; k < 2; ++k) {
      pp[2 * k] = pool_args(*PS[k], br[k].S1, nS, 32, nS1, br[k].S1p);
      pp[2 * k + 1] = pool_args(*PT[k], br[k].T1, nT, 32, nT1, br[k].T1p);
    }
    launch_pools(pp, 4, B, s);
    // layer 2 on the pooled graphs; master = the first layer's master output
    for (int k = 0; k < 2; ++k) {
      pr[2 * k] = proj_args(*H2[k], false, br[k].T1p, nT1, nT1 + nS1, 0, br[k].xp2);
      pr[2 * k + 1] = proj_args(*H2[k], true, br[k].S1p, nS1, nT1 + nS1, nT1, br[k].xp2);
      ga[k] = hgat_args(*H2[k], nT1, nS1, br[k].xp2, br[k].m1, 32, br[k].Ta, br[k].Sa, br[k].ma);
    }
    launch_rowlins(pr, 4, s);
    AOK(launch_gat(ga[0], B, H2[0]->din, H2[0]->dout, s, &ga[1]));
  }
  {  // debug views for afx_tap
    int n = 0;
    auto dbg = [&](const char* nm, const float* ptr, size_t cnt) { ws.dbg_name[n] = nm; ws.dbg_ptr[n] = ptr; ws.dbg_n[n] = cnt; ++n; };
    dbg("gat_S", ws.gS, (size_t)B * AAS_F * 64); dbg("gat_T", ws.gT, (size_t)B * wd * 64);
    dbg("out_S", ws.oS, (size_t)B * nS * 64); dbg("out_T", ws.oT, (size_t)B * nT * 64);
    dbg("b1_T1", br[0].T1, (size_t)B * nT * 32); dbg("b1_S1", br[0].S1, (size_t)B * nS * 32); dbg("b1_m1", br[0].m1, (size_t)B * 32);
    dbg("b1_T1p", br[0].T1p, (size_t)B * nT1 * 32); dbg("b1_S1p", br[0].S1p, (size_t)B * nS1 * 32);
    dbg("b1_Ta", br[0].Ta, (size_t)B * nT1 * 32); dbg("b1_Sa", br[0].Sa, (size_t)B * nS1 * 32); dbg("b1_ma", br[0].ma, (size_t)B * 32);
    dbg("b2_T1", br[1].T1, (size_t)B * nT * 32); dbg("b2_S1", br[1].S1, (size_t)B * nS * 32); dbg("b2_m1", br[1].m1, (size_t)B * 32);
    dbg("b2_T1p", br[1].T1p, (size_t)B * nT1 * 32); dbg("b2_S1p", br[1].S1p, (size_t)B * nS1 * 32);
    dbg("b2_Ta", br[1].Ta, (size_t)B * nT1 * 32); dbg("b2_Sa", br[1].Sa, (size_t)B * nS1 * 32); dbg("b2_ma", br[1].ma, (size_t)B * 32);
    dbg("b1_xp", br[0].xp, (size_t)B * (nT + nS) * 64); dbg("b1_xp2", br[0].xp2, (size_t)B * (nT1 + nS1) * 32);
    dbg("b2_xp", br[1].xp, (size_t)B * (nT + nS) * 64); dbg("b2_xp2", br[1].xp2, (size_t)B * (nT1 + nS1) * 32);
    ws.dbg_count = n;
  }
  hipLaunchKernelGGL(readout_kernel, dim3(B), dim3(32), 0, s, br[0].T1p, br[0].Ta, br[0].S1p, br[0].m1, br[0].ma,
                     br[1].T1p, br[1].Ta, br[1].S1p, br[1].Sa, br[1].m1, br[1].ma, nT1, nS1, w.out_w, w.out_b,
                     ws.hidden, logits, nonfinite);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
#undef ATAP
}

}  // namespace afx

// ===================================================================================
// single-module C entry points (unit parity against the reference's own modules)
// ===================================================================================
namespace afx {
__global__ void node_mean_kernel(const float* x, int N, int D, float* out) {
  const int b = blockIdx.x, d = threadIdx.x;
  if (d >= D) return;
  float a = 0.f;
  for (int j = 0; j < N; ++j) a += x[((long)b * N + j) * D + d];
  out[(long)b * D + d] = a / (float)N;
}
const char* aasist_last = nullptr;
}  // namespace afx

extern "C" const char* afx_aasist_error(void) { return afx::aasist_last ? afx::aasist_last : ""; }

extern "C" int afx_k_gat(const float* x, int B, int N, int din, int dout, const float* att_w, const float* att_b,
                         const float* att_vec, const float* w1, const float* b1, const float* w2, const float* b2,
                         const float* bn_scale, const float* bn_shift, float temp, float* y, void* stream) {
  using namespace afx;
  GatArgs a;
  memset(&a, 0, sizeof a);
  a.x = x; a.N = N; a.n1 = N; a.att_w = att_w; a.att_b = att_b; a.v11 = a.v22 = a.v12 = att_vec;
  a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2; a.bn_scale = bn_scale; a.bn_shift = bn_shift; a.temp = temp;
  a.y1 = y; a.y2 = y;
  aasist_last = launch_gat(a, B, din, dout, (hipStream_t)stream);
  return aasist_last ? 1 : 0;
}

extern "C" int afx_k_hgat(const float* x1, int n1, const float* x2, int n2, int B, int din, int dout,
                          const float* const* wts /* 22 pointers, order below */, float temp, const float* master,
                          long master_bstride, float* xp_scratch /* B*(n1+n2)*din + B*din */, float* y1, float* y2,
                          float* mout, void* stream) {
  using namespace afx;
  // wts: t1w t1b t2w t2b att_w att_b attM_w attM_b v11 v22 v12 vM w1 b1 w2 b2 w1M b1M w2M b2M bn_scale bn_shift
  hipStream_t s = (hipStream_t)stream;
  const int N = n1 + n2;
  const RowlinArgs pr[2] = {{x1, (long)din, B * n1, din, wts[0], wts[1], din, xp_scratch, (long)din, n1, N, 0},
                            {x2, (long)din, B * n2, din, wts[2], wts[3], din, xp_scratch, (long)din, n2, N, n1}};
  launch_rowlins(pr, 2, s);
  if (!master) {  // models/aasist_modules.py:167-168: mean of the projected nodes
    float* mean = xp_scratch + (long)B * N * din;
    hipLaunchKernelGGL(node_mean_kernel, dim3(B), dim3(64), 0, s, xp_scratch, N, din, mean);
    master = mean;
    master_bstride = din;
  }
  GatArgs a;
  memset(&a, 0, sizeof a);
  a.x = xp_scratch; a.N = N; a.n1 = n1; a.att_w = wts[4]; a.att_b = wts[5]; a.attM_w = wts[6]; a.attM_b = wts[7];
  a.v11 = wts[8]; a.v22 = wts[9]; a.v12 = wts[10]; a.vM = wts[11];
  a.w1 = wts[12]; a.b1 = wts[13]; a.w2 = wts[14]; a.b2 = wts[15];
  a.w1M = wts[16]; a.b1M = wts[17]; a.w2M = wts[18]; a.b2M = wts[19];
  a.bn_scale = wts[20]; a.bn_shift = wts[21]; a.temp = temp; a.y1 = y1; a.y2 = y2;
  a.master = master; a.master_bstride = master_bstride; a.master_out = mout;
  aasist_last = launch_gat(a, B, din, dout, s);
  return aasist_last ? 1 : 0;
}

// ---- Residual_block alone (models/aasist_modules.py:340-397) on an NCHW image of any size: the same kernels as
// the fused front (zero-padded channel-last image, convs as chunked-K products on the fp32 matrix cores) between
// two layout passes.  conv1 sees x itself (Q2: the bn1 + SELU result is discarded by the reference).
namespace afx {
__global__ void nchw_to_img_kernel(const float* __restrict__ x, int C, int H, int W, int hp, int wp, float* __restrict__ img,
                                   long total) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int w = (int)(i % W), h = (int)(i / W % H), c = (int)(i / ((long)W * H) % C);
    const long b = i / ((long)W * H * C);
    img[((b * hp + h + 1) * wp + w + 1) * C + c] = x[i];
  }
}
__global__ void img_to_nchw_kernel(const float* __restrict__ img, int C, int H, int W, int hp, int wp, float* __restrict__ y,
                                   long total) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int w = (int)(i % W), h = (int)(i / W % H), c = (int)(i / ((long)W * H) % C);
    const long b = i / ((long)W * H * C);
    y[i] = img[((b * hp + h + 1) * wp + w + 1) * C + c];
  }
}
}  // namespace afx

extern "C" size_t afx_k_resblock_scratch_floats(int B, int cin, int cout, int H, int W) {
  const size_t pix = (size_t)B * (H + 4) * (W + 2) + 3 * (size_t)(W + 2) + 16;
  return pix * ((size_t)cin + 3 * (size_t)cout) + (size_t)cout * cin * 6 + (size_t)cout * cout * 6 + (size_t)cout * cin * 3 + 256;
}

extern "C" int afx_k_resblock(const float* x, int B, int cin, int cout, int H, int W, const float* conv1_w,
                              const float* conv1_b, const float* bn2_scale, const float* bn2_shift, const float* conv2_w,
                              const float* conv2_b, const float* down_w, const float* down_b, float* scratch, float* y,
                              void* stream) {
  using namespace afx;
  hipStream_t s = (hipStream_t)stream;
  auto bad = [&](const char* m) { aasist_last = m; return 1; };
  if (!x || !conv1_w || !conv1_b || !bn2_scale || !bn2_shift || !conv2_w || !conv2_b || !scratch || !y) return bad("resblock: null argument");
  if (B < 1 || H < 1 || W < 1) return bad("resblock: empty image");
  if (cout != 32 && cout != 64 && cout != 128) return bad("resblock: output channels must be 32, 64 or 128");
  if (cin != 1 && cin % 16) return bad("resblock: input channels must be 1 or a multiple of 16");
  if ((cin != cout) != (down_w != nullptr)) return bad("resblock: conv_downsample exactly when the channel count changes");
  const int hp = H + 4, wp = W + 2, img = hp * wp;
  const long M = (long)B * img;
  const size_t pix = (size_t)M + 3 * (size_t)wp + 16;
  float* X = scratch;
  float* Y = X + pix * cin;
  float* D = Y + pix * cout;
  float* O = D + pix * cout;
  float* w1p = O + pix * cout;
  float* w2p = w1p + (size_t)cout * cin * 6;
  float* wdp = w2p + (size_t)cout * cout * 6;
  if (hipMemsetAsync(scratch, 0, pix * ((size_t)cin + 3 * (size_t)cout) * 4, s) != hipSuccess) return bad("resblock: memset failed");
  hipLaunchKernelGGL(pack_conv2d_kernel, dim3(64), dim3(256), 0, s, conv1_w, cout, cin, 2, 3, w1p);
  hipLaunchKernelGGL(pack_conv2d_kernel, dim3(64), dim3(256), 0, s, conv2_w, cout, cout, 2, 3, w2p);
  if (down_w) hipLaunchKernelGGL(pack_conv2d_kernel, dim3(64), dim3(256), 0, s, down_w, cout, cin, 1, 3, wdp);
  const long nin = (long)B * cin * H * W, nout = (long)B * cout * H * W;
  hipLaunchKernelGGL(nchw_to_img_kernel, dim3((unsigned)((nin + 255) / 256 < 4096 ? (nin + 255) / 256 : 4096)), dim3(256), 0, s, x,
                     cin, H, W, hp, wp, X, nin);
  F32GemmArgs g;
  const float* resid = X;
  if (cin == 1) {  // conv1 + bn2 + SELU -> Y and the (1,3) downsample -> D in one VALU kernel (K = 6 / 3: no matrix shape)
    const long n = M * cout;
    hipLaunchKernelGGL(first_block_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, X, (int)M, img, wp, W, w1p, conv1_b,
                       bn2_scale, bn2_shift, wdp, down_b, Y, D, cout, H);
    resid = D;
  } else {
    memset(&g, 0, sizeof g);  // conv1 (pad (1,1)) on x -> bn2 -> SELU -> Y, H + 1 rows
    g.A = X; g.lda = cin; g.nch = 2; g.kc = 3 * cin; g.chunk_stride = (long)wp * cin;
    g.W = w1p; g.M = (int)M; g.N = cout; g.bias = conv1_b; g.bn_scale = bn2_scale; g.bn_shift = bn2_shift; g.post = 1;
    g.img = img; g.wp = wp; g.hout = H + 1; g.wd = W; g.out = Y; g.ldo = cout; g.o_off = wp + 1;
    if ((aasist_last = launch_f32_gemm(g, s))) return 1;
    if (down_w) {
      memset(&g, 0, sizeof g);
      g.A = X + (long)wp * cin; g.lda = cin; g.nch = 1; g.kc = 3 * cin; g.W = wdp; g.M = (int)M; g.N = cout;
      g.bias = down_b; g.img = img; g.wp = wp; g.hout = H; g.wd = W; g.out = D; g.ldo = cout; g.o_off = wp + 1;
      if ((aasist_last = launch_f32_gemm(g, s))) return 1;
      resid = D;
    }
  }
  memset(&g, 0, sizeof g);  // conv2 (pad (0,1)) on Y + identity
  g.A = Y + (long)wp * cout; g.lda = cout; g.nch = 2; g.kc = 3 * cout; g.chunk_stride = (long)wp * cout;
  g.W = w2p; g.M = (int)M; g.N = cout; g.bias = conv2_b; g.resid = resid;
  g.img = img; g.wp = wp; g.hout = H; g.wd = W; g.out = O; g.ldo = cout; g.o_off = wp + 1;
  if ((aasist_last = launch_f32_gemm(g, s))) return 1;
  hipLaunchKernelGGL(img_to_nchw_kernel, dim3((unsigned)((nout + 255) / 256 < 4096 ? (nout + 255) / 256 : 4096)), dim3(256), 0, s, O,
                     cout, H, W, hp, wp, y, nout);
  hipError_t e = hipGetLastError();
  aasist_last = e == hipSuccess ? nullptr : hipGetErrorString(e);
  return aasist_last ? 1 : 0;
}

extern "C" int afx_k_graph_pool(const float* h, int B, int N, int D, int keep, const float* w, const float* b,
                                float* out, void* stream) {
  using namespace afx;
  if (N < 1 || N > 1024 || keep < 1 || keep > N) {
    aasist_last = "graph_pool: need 1 <= keep <= N <= 1024";
    return 1;
  }
  const PoolArgs pq = {h, N, D, keep, w, b, out};
  launch_pools(&pq, 1, B, (hipStream_t)stream);
  hipError_t e = hipGetLastError();
  aasist_last = e == hipSuccess ? nullptr : hipGetErrorString(e);
  return aasist_last ? 1 : 0;
}
