// Transformer self-attention for the SSL trunk, gfx950.
// T <= 224 frames (4-s clips give T = 199..201), head dim 64: one workgroup per
// (utterance, head) keeps that head's whole K (row-major, XOR-swizzled 128-B rows)
// and V^T (keys contiguous) in LDS -- 57 KB -- and its 4 waves walk the 16-row query
// tiles.  Per query tile:
//   S^T = K Q^T   via v_mfma 16x16x32 with K as the A-operand, so a lane owns one
//                 query row (lane&15) and keys 16*kt + 4*(lane>>4) + 0..3;
//   softmax       in registers: lane-local max/sum + two xor-shuffles (lanes 16/32
//                 apart share the row); masked keys contribute exactly 0;
//   O^T = V^T P^T the S^T accumulator layout is re-used directly as the B-operand
//                 (k-slots permuted identically on the V^T side), no LDS round trip;
//                 the lane keeps its query row, so normalisation is lane-local and the
//                 output leaves as 16-B stores.
// Q never touches LDS (each wave reads its own 16 rows as 16-B fragments).
#include "afx_common.h"
#include "afx_kernels.h"

#ifndef MHSA_DBG
#define MHSA_DBG 0  // timing experiments only (wrong results): 1 no K/V staging, 2 no query-tile loop, 4 no V^T scatter, 8 no exp, 16 no P.V, 32 no Q.K^T, 64 no stores
#endif

namespace afx {

constexpr int ATT_KEYS = 224;       // padded key capacity (7 k-steps of 32)
constexpr int ATT_VT_STRIDE = 232;  // halfs per V^T row: 464 B, conflict-free ds_read_b64

// NW waves per workgroup: the 16-query tiles of a head are dealt to the waves round-robin, so the compute phase is
// ceil(tiles / NW) tiles long -- 13 tiles (T = 199): 4 with four waves, 2 with seven (and 1 when the tiles are split over
// two workgroups, B x H < 256); the staging loop is spread over all threads.
// RING (the KV-cached streaming mode, afx_kv_step -- NOT a reference function): `qkv` is a per-stream ring of KS*32 slots
// (q | k | v rows as the QKV product wrote them) in 16-slot groups, one group per 250-ms chunk; group gidx holds ring.cnt[gidx]
// valid frames (the rest of its slots, and groups never written, are masked).  Attention has no positional term, so the
// order of the keys in the ring does not matter: the ONE query tile ring.q_tile (the newest chunk's group) attends to every
// valid slot -- its own chunk and the cached K / V of the chunks before it.  Output row = slot - 16 q_tile of a 16-row
// block per stream.
struct MhsaRing {
  int q_tile;
  unsigned char cnt[16];
};
// RING == 2 (per-stream sessions, afx_kv_step_ragged): the valid counts come per stream from a device table instead of
// ring.cnt -- `lens` then points at (S, 8) ints per stream: [0] = the stream's base group (the group of its first chunk),
// ints [4, 8) = its 16 valid counts as bytes -- and the 256 slots are visited rotated by the base group: key i is slot
// (((i >> 4) + base) & 15) * 16 + (i & 15).  Key and summation order are then those of a stream that started at group 0.
// RING == 3 (a step over a list of active streams, afx_kv_step_active): as RING == 2, with `lens` a compact (A, 8) table
// whose row b also names the stream -- [1] its newest group (the query tile), [2] its index among the S rings -- so
// blockIdx.y walks the list and output row b is list entry b's.
// (read where it is used, as ring.q_tile always was: the RING < 3 forms compile to the instructions they had)
#define ring_qtile (RING == 3 ? lens[(long)b * 8 + 1] : ring.q_tile)
__device__ __forceinline__ int ring_slot(int key, int base) { return ((((key >> 4) + base) & 15) << 4) | (key & 15); }
// VTR (round 3): V stays ROW-major in LDS (staged exactly like K: one swizzled 16-byte write per loaded chunk, no transposing
// scatter) and the V^T fragments of P.V come from `ds_read_b64_tr_b16` -- per 16-lane group a block of 4 keys x 16 dims delivered
// column-major, i.e. lane (dim) gets its 4 consecutive keys, the same registers the V^T image gave.
template <class HT, int KS, int NW, int RING = 0, bool VTR = false>  // KS = number of 32-key steps actually computed
__global__ __launch_bounds__(64 * NW, NW > 4 ? 4 : 2) void mhsa_kernel(const typename HT::T* __restrict__ qkv,
                                                   typename HT::T* __restrict__ out, int T, int H, float scale,
                                                   const int* __restrict__ lens, MhsaRing ring) {
  constexpr int ATT_KEYS = KS <= 7 ? afx::ATT_KEYS : KS * 32;             // (shadow the file-level capacity: 8 steps = 256 slots)
  constexpr int ATT_VT_STRIDE = KS <= 7 ? afx::ATT_VT_STRIDE : KS * 32 + 8;  // 264 halfs = 132 words: conflict-free as 116 is
  typedef typename HT::T Tt;
  typedef typename HT::V8 V8;
  typedef typename HT::V4 V4;
  constexpr int NKT = KS * 2;     // 16-key tiles
  constexpr int KEYS = KS * 32;   // keys covered
  __shared__ __attribute__((aligned(16))) char k_lds[ATT_KEYS * 128];
  __shared__ __attribute__((aligned(16))) Tt vt_lds[VTR ? ATT_KEYS * 64 : 64 * ATT_VT_STRIDE];  // VTR: [key][64 dims], chunk c at c ^ (key & 7)
  __shared__ __attribute__((aligned(16))) float mask_lds[ATT_KEYS];  // 0 for a key of this utterance, -1e30 beyond it

  const int h = blockIdx.x, b = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long ld = 3L * H * 64;
  // Ragged batch (key-padding mask): utterance b has lens[b] valid frames of the Trow rows it owns in memory; from
  // here on T is ITS length -- keys beyond it are staged as zeros and masked, queries beyond it are not computed.
  const int Trow = T;
  if (RING < 2 && lens) T = lens[b];
  const unsigned char* scnt = RING >= 2 ? (const unsigned char*)(lens + (long)b * 8 + 4) : nullptr;
  const int sbase = RING >= 2 ? lens[(long)b * 8] : 0;
  // RING == 3 (afx_kv_step_active): row b of the table belongs to the active stream lens[8 b + 2], whose newest chunk
  // sits in ITS OWN group lens[8 b + 1] (ring_qtile); the output stays row b
  const Tt* base = qkv + (long)(RING == 3 ? lens[(long)b * 8 + 2] : b) * Trow * ld + h * 64;
  const Tt* kbase = base + (long)H * 64;
  const Tt* vbase = base + 2L * H * 64;

  // ---- stage K (swizzled rows) and V^T ------------------------------------------
  // all global loads of the thread first, then the LDS writes: issued one (load, wait, write) step at a
  // time the staging was 7 dependent L2 round trips and most of this kernel's time
  {
    constexpr int NT = 64 * NW;
    constexpr int IT = KEYS * 8 / NT;
    static_assert(KEYS * 8 % NT == 0, "staging loop shape");
    u32x4 kreg[IT];
    V8 vreg[IT];
    // thread -> 16-byte column c of IT CONSECUTIVE keys (kg IT .. kg IT + IT - 1): the V^T image then takes one IT-key vector
    // per dimension (8 writes of 2 IT bytes per thread) instead of 8 IT two-byte scatters
    const int c = tid & 7, kg = tid >> 3;
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int key = kg * IT + it;
      kreg[it] = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
      for (int i = 0; i < 8; ++i) vreg[it][i] = (Tt)0.f;
      const int slot = RING >= 2 ? ring_slot(key, sbase) : key;
      const bool live = RING >= 2 ? (slot & 15) < scnt[slot >> 4] : RING ? (key & 15) < ring.cnt[(key >> 4) & 15] : key < T;
      if (live && !(MHSA_DBG & 1)) {
        kreg[it] = *(const u32x4*)(kbase + (long)slot * ld + c * 8);
        vreg[it] = *(const V8*)(vbase + (long)slot * ld + c * 8);
      }
    }
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int key = kg * IT + it;
      *(u32x4*)(k_lds + key * 128 + ((c ^ ((key >> 1) & 7)) * 16)) = kreg[it];
    }
    if constexpr (VTR) {
#pragma unroll
      for (int it = 0; it < IT; ++it) {
        const int key = kg * IT + it;
        *(V8*)((char*)vt_lds + key * 128 + ((c ^ (key & 7)) * 16)) = vreg[it];
      }
    } else if (!(MHSA_DBG & 4)) {
      if constexpr (IT == 2 || IT == 4 || IT == 8) {
        typedef Tt __attribute__((ext_vector_type(IT))) VK;
        static_assert(ATT_VT_STRIDE % IT == 0, "V^T rows keep the key vectors aligned");
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          VK col;
#pragma unroll
          for (int it = 0; it < IT; ++it) col[it] = vreg[it][i];
          *(VK*)(vt_lds + (c * 8 + i) * ATT_VT_STRIDE + kg * IT) = col;
        }
      } else {  // (the 4-wave A/B instance at 224 keys: 7 keys per thread, element by element)
#pragma unroll
        for (int it = 0; it < IT; ++it)
#pragma unroll
          for (int i = 0; i < 8; ++i) vt_lds[(c * 8 + i) * ATT_VT_STRIDE + kg * IT + it] = vreg[it][i];
      }
    }
  }
  for (int i = tid; i < KEYS; i += 64 * NW)
    mask_lds[i] = (RING >= 2 ? (i & 15) < scnt[ring_slot(i, sbase) >> 4] : RING ? (i & 15) < ring.cnt[(i >> 4) & 15] : i < T) ? 0.f : -1e30f;
  __syncthreads();
  if (MHSA_DBG & 2) return;

  const int ql = lane & 15, g = lane >> 4;
  // gridDim.z splits the query tiles of one (utterance, head) over several workgroups (each stages K / V itself):
  // at small batches B x H workgroups do not fill the chip (B = 16: 256 of them for 256 CUs x 2 slots)
  const int nqt_all = (T + 15) >> 4;
  const int per_z = (nqt_all + (int)gridDim.z - 1) / (int)gridDim.z;
  const int qt_first = RING ? ring_qtile : (int)blockIdx.z * per_z;
  const int nqt = RING ? ring_qtile + 1 : min(nqt_all, qt_first + per_z);
  auto load_q = [&](int qt, V8 (&f)[2]) {
    int qrow = qt * 16 + ql;
    qrow = qrow < T ? qrow : T - 1;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) f[ks] = *(const V8*)(base + (long)qrow * ld + ks * 32 + g * 8);
  };
  V8 qnext[2];
  if (qt_first + wave < nqt) load_q(qt_first + wave, qnext);
  for (int qt = qt_first + wave; qt < nqt; qt += NW) {
    const int q0 = qt * 16;
    V8 qf[2] = {qnext[0], qnext[1]};
    if (qt + NW < nqt) load_q(qt + NW, qnext);  // the next tile's Q rows are in flight under this tile's work

    // S^T tiles: s[kt][r] = S[q0+ql][16kt + 4g + r].  Two key tiles at a time (4 fragment reads in
    // flight, then 4 MFMAs on two accumulators): the sched_barriers stop hipcc from hoisting all 28
    // reads to the top, which cost 360 VGPRs and left one workgroup per CU.
    f32x4 s[NKT];
    auto read_k = [&](int kp, V8 (&kf)[2][2]) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int krow = (kp + u) * 16 + ql;
        const int sw = (krow >> 1) & 7;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) kf[u][ks] = *(const V8*)(k_lds + krow * 128 + (((ks * 4 + g) ^ sw) * 16));
      }
    };
    V8 kfa[2][2], kfb[2][2];
    read_k(0, kfa);
#pragma unroll
    for (int kp = 0; kp < NKT; kp += 2) {
      // the next pair's fragments are requested before this pair's MFMAs (counted lgkmcnt keeps them in flight)
      V8(&cur)[2][2] = (kp & 2) ? kfb : kfa;
      V8(&nxt)[2][2] = (kp & 2) ? kfa : kfb;
      if (kp + 2 < NKT) read_k(kp + 2, nxt);
      __builtin_amdgcn_sched_barrier(0);
      // the accumulators START at the key mask (0 / -1e30: one 16-B LDS read per tile, issued with the K fragments)
      // instead of at zero: keys past the utterance's length (their K rows are staged as zeros, so q.k adds 0) come
      // out of the MFMAs already masked -- no compare / select per score
#pragma unroll
      for (int u = 0; u < 2; ++u) s[kp + u] = *(const f32x4*)(mask_lds + (kp + u) * 16 + g * 4);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          if (MHSA_DBG & 32) asm volatile("" :: "v"(cur[u][ks]));
          else s[kp + u] = HT::mfma(cur[u][ks], qf[ks], s[kp + u]);
        }
      __builtin_amdgcn_sched_barrier(0);
    }
    // softmax over the keys, in the exp2 domain on the RAW scores: the row maximum does not care about the positive
    // scale, and exp(scale (s - max)) = exp2((s - max) scale log2 e) is one fma + one v_exp per element.  (The first
    // version scaled, masked and subtracted per element -- ~9 VALU slots each, 56 elements per lane per query tile:
    // the softmax, not the 56 MFMAs, was most of this kernel's compute phase.)
    const float c2 = scale * 1.4426950408889634f;
    float mx = -1e30f;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[kt][r]);
    mx = rows_max(mx);
    const float mc = -mx * c2;
    float sum = 0.f;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float a = fmaf(s[kt][r], c2, mc);
        const float e = (MHSA_DBG & 8) ? a : __builtin_amdgcn_exp2f(a);
        s[kt][r] = e;
        sum += e;
      }
    sum = rows_sum(sum);
    const float rinv = 1.0f / sum;
    // O = P V : k-slot (g, jj) of step s2 <-> key 32*s2 + 16*(jj>>2) + 4g + (jj&3)
    f32x4 o[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) o[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto read_v = [&](int s2, V8 (&vf)[4]) {
      if constexpr (VTR) {
        // lane 4q + p of a 16-lane group supplies the address of key (block + q), dims 16 nt + 4p .. + 3; the group's lane i
        // receives dim 16 nt + i of the block's 4 keys.  Blocks: keys 32 s2 + 4g .. + 3 (lo) and 16 beyond (hi).
        typedef short tr4 __attribute__((__vector_size__(4 * sizeof(short))));
        const int tq = ql >> 2, tp = ql & 3;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
          const int chunk = nt * 2 + (tp >> 1);
          const int k_lo = s2 * 32 + g * 4 + tq, k_hi = k_lo + 16;
          const char* alo = (const char*)vt_lds + k_lo * 128 + ((chunk ^ (k_lo & 7)) * 16) + (tp & 1) * 8;
          const char* ahi = (const char*)vt_lds + k_hi * 128 + ((chunk ^ (k_hi & 7)) * 16) + (tp & 1) * 8;
          const tr4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) tr4*)alo);
          const tr4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) tr4*)ahi);
          union { tr4 v[2]; V8 f; } u;
          u.v[0] = lo;
          u.v[1] = hi;
          vf[nt] = u.f;
        }
      } else {
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const Tt* vr = vt_lds + (nt * 16 + ql) * ATT_VT_STRIDE + s2 * 32 + g * 4;
        const V4 lo = *(const V4*)vr;
        const V4 hi = *(const V4*)(vr + 16);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          vf[nt][r] = lo[r];
          vf[nt][4 + r] = hi[r];
        }
      }
      }
    };
    V8 vfa[4], vfb[4];
    read_v(0, vfa);
#pragma unroll
    for (int s2 = 0; s2 < KS; ++s2) {
      V8(&cur)[4] = (s2 & 1) ? vfb : vfa;
      V8(&nxt)[4] = (s2 & 1) ? vfa : vfb;
      if (s2 + 1 < KS) read_v(s2 + 1, nxt);
      V8 pf;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        pf[r] = (Tt)s[2 * s2][r];
        pf[4 + r] = (Tt)s[2 * s2 + 1][r];
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {  // O^T = V^T P^T: the lane keeps ONE query row
        if (MHSA_DBG & 16) asm volatile("" :: "v"(cur[nt]), "v"(pf));
        else o[nt] = HT::mfma(cur[nt], pf, o[nt]);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    // o[nt][r] = O[q0 + ql][16nt + 4g + r]: 4 consecutive head dims of the lane's own query row,
    // so the row's 1/sum is already local.  v_permlane16_swap pairs the two 16-column tiles
    // (as in the GEMM epilogue) -> each lane stores 8 consecutive dims (16 B).
    const int q = q0 + ql;
    const int cb = (g & 1) * 16 + (g >> 1) * 8;
#pragma unroll
    for (int np = 0; np < 2; ++np) {
      f32x4 va = o[2 * np] * rinv, vb = o[2 * np + 1] * rinv;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(va[r]), __float_as_uint(vb[r]), false, false);
        va[r] = __uint_as_float(sw[0]);
        vb[r] = __uint_as_float(sw[1]);
      }
      if (MHSA_DBG & 64) {
        asm volatile("" :: "v"(va), "v"(vb));
      } else if (q < T) {
        V8 hv;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          hv[r] = (Tt)va[r];
          hv[4 + r] = (Tt)vb[r];
        }
        const long orow = RING ? (long)b * 16 + (q - 16 * ring_qtile) : (long)b * Trow + q;
        *(V8*)(out + orow * (H * 64) + h * 64 + np * 32 + cb) = hv;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------
// Split-precision form of the one-pass kernel (the engine's dtype "fp16x3": fp32 q | k | v rows in, fp32 rows out; every
// product on the fp16 matrix pipe as hi.hi + lo.hi + hi.lo of fp16 hi / lo operand pairs, ~22 significant bits):
//   S^T = Kh Qh^T + Kh Ql^T + Kl Qh^T        (K staged as a hi and a lo image, Q split in registers)
//   O^T = Vh^T Ph^T + Vh^T Pl^T + Vl^T Ph^T  (P in [0, 1] split after the fp32 softmax)
// Same work split, masks and softmax as mhsa_kernel; one workgroup per CU (114 KB of LDS: two K images, two V^T images).
// It replaces the fp32 VALU attention in that mode (93 -> ~20 us per layer at B = 16); exact mode ("fp32") keeps the VALU kernel.
// ---------------------------------------------------------------------------------------
// RING (round 4; the KV-cached streaming mode in dtype "fp16x3" -- NOT a reference function, see mhsa_kernel's RING): `qkv` is the
// per-stream ring of 256 fp32 [q | k | v] slots in 16-slot groups; the ONE query tile ring.q_tile attends to every valid slot.
template <int KS, int NW, int RING = 0>
__global__ __launch_bounds__(64 * NW, 2) void mhsa_split_kernel(const float* __restrict__ qkv, float* __restrict__ out, int T, int H,
                                                                 float scale, const int* __restrict__ lens, int out_pairs, float out_scale,
                                                                 MhsaRing ring) {
  typedef _Float16 Tt;
  typedef f16x8 V8;
  typedef f16x4 V4;
  constexpr int NKT = KS * 2, KEYS = KS * 32;
  constexpr int ATT_KEYS = KS <= 7 ? afx::ATT_KEYS : KS * 32;                 // (8 steps = the ring's 256 slots)
  __shared__ __attribute__((aligned(16))) char k_lds[2][ATT_KEYS * 128];        // [hi / lo][key][64 halfs], swizzled rows
  __shared__ __attribute__((aligned(16))) Tt vt_lds[2][ATT_KEYS * 64];          // [hi / lo][key][64 dims], chunk c at c ^ (key & 7): V stays
                                                                                // row-major, the PV fragments are transposing reads (mhsa_kernel's VTR)
  __shared__ __attribute__((aligned(16))) float mask_lds[ATT_KEYS];
  const int h = blockIdx.x, b = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long ld = 3L * H * 64;
  const int Trow = T;
  if (RING < 2 && lens) T = lens[b];
  const unsigned char* scnt = RING >= 2 ? (const unsigned char*)(lens + (long)b * 8 + 4) : nullptr;
  const int sbase = RING >= 2 ? lens[(long)b * 8] : 0;
  // RING == 3 (afx_kv_step_active): row b of the table belongs to the active stream lens[8 b + 2], whose newest chunk
  // sits in ITS OWN group lens[8 b + 1] (ring_qtile); the output stays row b
  const float* base = qkv + (long)(RING == 3 ? lens[(long)b * 8 + 2] : b) * Trow * ld + h * 64;
  const float* kbase = base + (long)H * 64;
  const float* vbase = base + 2L * H * 64;
  auto split8 = [](const f32x4& a, const f32x4& c, V8& hi, V8& lo) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      hi[r] = (Tt)a[r];
      hi[4 + r] = (Tt)c[r];
      lo[r] = (Tt)(a[r] - (float)hi[r]);
      lo[4 + r] = (Tt)(c[r] - (float)hi[4 + r]);
    }
  };
  // ---- stage K (hi, lo; swizzled rows) and V^T (hi, lo) --------------------------------
  {
    constexpr int NT = 64 * NW;
    for (int idx = tid; idx < KEYS * 8; idx += NT) {
      const int key = idx >> 3, c = idx & 7;
      f32x4 k0 = f32x4{0.f, 0.f, 0.f, 0.f}, k1 = k0, v0 = k0, v1 = k0;
      const int slot = RING >= 2 ? ring_slot(key, sbase) : key;
      if (RING >= 2 ? (slot & 15) < scnt[slot >> 4] : RING ? (key & 15) < ring.cnt[(key >> 4) & 15] : key < T) {
        k0 = *(const f32x4*)(kbase + (long)slot * ld + c * 8);
        k1 = *(const f32x4*)(kbase + (long)slot * ld + c * 8 + 4);
        v0 = *(const f32x4*)(vbase + (long)slot * ld + c * 8);
        v1 = *(const f32x4*)(vbase + (long)slot * ld + c * 8 + 4);
      }
      V8 kh, kl, vh, vl;
      split8(k0, k1, kh, kl);
      split8(v0, v1, vh, vl);
      const int off = key * 128 + ((c ^ ((key >> 1) & 7)) * 16);
      *(V8*)(k_lds[0] + off) = kh;
      *(V8*)(k_lds[1] + off) = kl;
      const int voff = key * 128 + ((c ^ (key & 7)) * 16);
      *(V8*)((char*)vt_lds[0] + voff) = vh;
      *(V8*)((char*)vt_lds[1] + voff) = vl;
    }
  }
  for (int i = tid; i < KEYS; i += 64 * NW)
    mask_lds[i] = (RING >= 2 ? (i & 15) < scnt[ring_slot(i, sbase) >> 4] : RING ? (i & 15) < ring.cnt[(i >> 4) & 15] : i < T) ? 0.f : -1e30f;
  __syncthreads();
  const int ql = lane & 15, g = lane >> 4;
  const int nqt_all = (T + 15) >> 4;
  const int per_z = (nqt_all + (int)gridDim.z - 1) / (int)gridDim.z;
  const int qt_first = RING ? ring_qtile : (int)blockIdx.z * per_z;
  const int nqt = RING ? ring_qtile + 1 : min(nqt_all, qt_first + per_z);
  for (int qt = qt_first + wave; qt < nqt; qt += NW) {
    const int q0 = qt * 16;
    int qrow = q0 + ql;
    qrow = qrow < T ? qrow : T - 1;
    V8 qh[2], qlo[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const float* qp = base + (long)qrow * ld + ks * 32 + g * 8;
      split8(*(const f32x4*)qp, *(const f32x4*)(qp + 4), qh[ks], qlo[ks]);
    }
    f32x4 s[NKT];
    // one key tile's four fragments (hi / lo x two k-steps) are requested before the previous tile's six MFMAs (round 4, late: the
    // loop used to read, wait and multiply tile by tile -- 21.8 -> see DESIGN section 4); the sched_barriers keep hipcc from hoisting
    // all 56 fragment reads to the top (that spilled)
    auto read_k = [&](int kt, V8 (&kf)[2][2]) {
      const int krow = kt * 16 + ql, sw = (krow >> 1) & 7;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const int off = krow * 128 + (((ks * 4 + g) ^ sw) * 16);
        kf[ks][0] = *(const V8*)(k_lds[0] + off);
        kf[ks][1] = *(const V8*)(k_lds[1] + off);
      }
    };
    V8 kfa[2][2], kfb[2][2];
    read_k(0, kfa);
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
      V8(&cur)[2][2] = (kt & 1) ? kfb : kfa;
      V8(&nxt)[2][2] = (kt & 1) ? kfa : kfb;
      if (kt + 1 < NKT) read_k(kt + 1, nxt);
      s[kt] = *(const f32x4*)(mask_lds + kt * 16 + g * 4);  // the accumulators start at the key mask (0 / -1e30)
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        s[kt] = FP16::mfma(cur[ks][1], qh[ks], s[kt]);   // the small terms first, the large one last
        s[kt] = FP16::mfma(cur[ks][0], qlo[ks], s[kt]);
        s[kt] = FP16::mfma(cur[ks][0], qh[ks], s[kt]);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    const float c2 = scale * 1.4426950408889634f;
    float mx = -1e30f;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[kt][r]);
    mx = rows_max(mx);
    const float mc = -mx * c2;
    float sum = 0.f;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float e = __builtin_amdgcn_exp2f(fmaf(s[kt][r], c2, mc));
        s[kt][r] = e;
        sum += e;
      }
    sum = rows_sum(sum);
    const float rinv = 1.0f / sum;
    f32x4 o[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) o[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    // V fragments by transposing reads: lane 4q + p of a 16-lane group supplies the address of key (block + q), dims 16 nt + 4p .. + 3;
    // the group's lane i receives dim 16 nt + i of the block's 4 keys.  Blocks: keys 32 s2 + 4g .. + 3 (first four k-slots) and 16
    // beyond (last four).  The next 32-key step's eight fragments (hi / lo x four dim tiles) are requested before this step's MFMAs.
    auto read_v = [&](int s2, V8 (&vf)[4][2]) {
      typedef short tr4 __attribute__((__vector_size__(4 * sizeof(short))));
      const int tq = ql >> 2, tp = ql & 3;
      const int k_a = s2 * 32 + g * 4 + tq, k_b = k_a + 16;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const int chunk = nt * 2 + (tp >> 1);
        const int off_a = k_a * 128 + ((chunk ^ (k_a & 7)) * 16) + (tp & 1) * 8, off_b = k_b * 128 + ((chunk ^ (k_b & 7)) * 16) + (tp & 1) * 8;
#pragma unroll
        for (int hl = 0; hl < 2; ++hl) {
          const char* vb_ = (const char*)vt_lds[hl];
          union { tr4 v[2]; V8 f; } u;
          u.v[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) tr4*)(vb_ + off_a));
          u.v[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) tr4*)(vb_ + off_b));
          vf[nt][hl] = u.f;
        }
      }
    };
    V8 vfa[4][2], vfb[4][2];
    read_v(0, vfa);
#pragma unroll
    for (int s2 = 0; s2 < KS; ++s2) {
      V8(&cur)[4][2] = (s2 & 1) ? vfb : vfa;
      V8(&nxt)[4][2] = (s2 & 1) ? vfa : vfb;
      if (s2 + 1 < KS) read_v(s2 + 1, nxt);
      V8 ph, pl;
      split8(s[2 * s2], s[2 * s2 + 1], ph, pl);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        o[nt] = FP16::mfma(cur[nt][1], ph, o[nt]);
        o[nt] = FP16::mfma(cur[nt][0], pl, o[nt]);
        o[nt] = FP16::mfma(cur[nt][0], ph, o[nt]);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    const int q = q0 + ql;
    if (q < T) {
      const long eoff = (RING ? (long)b * 16 + (q - 16 * ring_qtile) : (long)b * Trow + q) * (H * 64) + h * 64;
      if (out_pairs) {  // the output projection's A operand: the pair form of out_scale x value in place of the fp32 row
        _Float16* hp = (_Float16*)out + 2 * eoff;  // (eoff % 64 == 0: a head's 64 columns are two whole 32-element groups)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
          f16x4 hi, lo;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float sv = o[nt][r] * rinv * out_scale;
            hi[r] = (_Float16)sv;
            lo[r] = (_Float16)(sv - (float)hi[r]);
          }
          const int po = (int)s3_pair_index(nt * 16 + g * 4);
          *(f16x4*)(hp + po) = hi;
          *(f16x4*)(hp + po + 32) = lo;
        }
      } else {
        float* orow = out + eoff;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) *(f32x4*)(orow + nt * 16 + g * 4) = o[nt] * rinv;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------
// The same attention for clips of ANY length (T > 224: the reference's test_duration_sec is a free
// config value, data/test_set.py:16,78,153): keys go through LDS in blocks of 128 with the usual running
// maximum / running sum per query row.  One workgroup = one (utterance, head, 64-query chunk); a wave
// keeps ONE 16-query tile (Q fragments, the 16 x 64 output accumulators and the row statistics stay in
// registers across all key blocks); per block it computes the 8 S^T tiles, rescales, and feeds the
// probabilities straight back as the B-operand of V^T P^T exactly as mhsa_kernel does.  LDS 33 KB.
// ---------------------------------------------------------------------------------------
constexpr int ATTL_KB = 128;         // keys per block
constexpr int ATTL_VT_STRIDE = 136;  // halfs per V^T row (68 words: conflict-free ds_read_b64 per half-wave)

template <class HT>
__global__ __launch_bounds__(256, 2) void mhsa_long_kernel(const typename HT::T* __restrict__ qkv,
                                                        typename HT::T* __restrict__ out, int T, int H, float scale,
                                                        const int* __restrict__ lens) {
  typedef typename HT::T Tt;
  typedef typename HT::V8 V8;
  typedef typename HT::V4 V4;
  constexpr int KS = ATTL_KB / 32, NKT = KS * 2;
  __shared__ __attribute__((aligned(16))) char k_lds[ATTL_KB * 128];
  __shared__ __attribute__((aligned(16))) Tt vt_lds[64 * ATTL_VT_STRIDE];
  const int h = blockIdx.x, b = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long ld = 3L * H * 64;
  const int Trow = T;  // ragged batch: see mhsa_kernel
  if (lens) T = lens[b];
  const Tt* base = qkv + (long)b * Trow * ld + h * 64;
  const Tt* kbase = base + (long)H * 64;
  const Tt* vbase = base + 2L * H * 64;
  const int ql = lane & 15, g = lane >> 4;
  const int q0 = blockIdx.z * 64 + wave * 16;
  const int q = q0 + ql;
  V8 qf[2];
  {
    const int qrow = q < T ? q : T - 1;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) qf[ks] = *(const V8*)(base + (long)qrow * ld + ks * 32 + g * 8);
  }
  float m = -1e30f, l = 0.f;
  f32x4 o[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) o[nt] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int j0 = 0; j0 < T; j0 += ATTL_KB) {
    if (j0) __syncthreads();  // every wave is done with the previous block
    {
      constexpr int IT = ATTL_KB * 8 / 256;
      u32x4 kreg[IT];
      V8 vreg[IT];
#pragma unroll
      for (int it = 0; it < IT; ++it) {
        const int idx = tid + it * 256, key = idx >> 3, c = idx & 7;
        kreg[it] = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < 8; ++i) vreg[it][i] = (Tt)0.f;
        if (j0 + key < T) {
          kreg[it] = *(const u32x4*)(kbase + (long)(j0 + key) * ld + c * 8);
          vreg[it] = *(const V8*)(vbase + (long)(j0 + key) * ld + c * 8);
        }
      }
#pragma unroll
      for (int it = 0; it < IT; ++it) {
        const int idx = tid + it * 256, key = idx >> 3, c = idx & 7;
        *(u32x4*)(k_lds + key * 128 + ((c ^ ((key >> 1) & 7)) * 16)) = kreg[it];
#pragma unroll
        for (int i = 0; i < 8; ++i) vt_lds[(c * 8 + i) * ATTL_VT_STRIDE + key] = vreg[it][i];
      }
    }
    __syncthreads();
    if (q0 >= T) continue;  // wave-uniform: a tile past the end only helps staging

    f32x4 s[NKT];
#pragma unroll
    for (int kp = 0; kp < NKT; kp += 2) {
      V8 kf[2][2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int krow = (kp + u) * 16 + ql;
        const int sw = (krow >> 1) & 7;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) kf[u][ks] = *(const V8*)(k_lds + krow * 128 + (((ks * 4 + g) ^ sw) * 16));
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) s[kp + u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int u = 0; u < 2; ++u) s[kp + u] = HT::mfma(kf[u][ks], qf[ks], s[kp + u]);
    }
    float bm = -1e30f;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = j0 + kt * 16 + g * 4 + r;
        const float v = key < T ? s[kt][r] * scale : -1e30f;
        s[kt][r] = v;
        bm = fmaxf(bm, v);
      }
    const float mn = fmaxf(m, rows_max(bm));
    const float corr = __expf(m - mn);
    float bl = 0.f;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float e = __expf(s[kt][r] - mn);
        s[kt][r] = e;
        bl += e;
      }
    l = fmaf(l, corr, rows_sum(bl));
    m = mn;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) o[nt] *= corr;
#pragma unroll
    for (int s2 = 0; s2 < KS; ++s2) {
      V8 vf[4];
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const Tt* vr = vt_lds + (nt * 16 + ql) * ATTL_VT_STRIDE + s2 * 32 + g * 4;
        const V4 lo = *(const V4*)vr;
        const V4 hi = *(const V4*)(vr + 16);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          vf[nt][r] = lo[r];
          vf[nt][4 + r] = hi[r];
        }
      }
      V8 pf;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        pf[r] = (Tt)s[2 * s2][r];
        pf[4 + r] = (Tt)s[2 * s2 + 1][r];
      }
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) o[nt] = HT::mfma(vf[nt], pf, o[nt]);
    }
  }
  if (q0 >= T) return;
  const float rinv = 1.0f / l;
  const int cb = (g & 1) * 16 + (g >> 1) * 8;
#pragma unroll
  for (int np = 0; np < 2; ++np) {
    f32x4 va = o[2 * np] * rinv, vb = o[2 * np + 1] * rinv;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(va[r]), __float_as_uint(vb[r]), false, false);
      va[r] = __uint_as_float(sw[0]);
      vb[r] = __uint_as_float(sw[1]);
    }
    if (q < T) {
      V8 hv;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        hv[r] = (Tt)va[r];
        hv[4 + r] = (Tt)vb[r];
      }
      *(V8*)(out + ((long)b * Trow + q) * (H * 64) + h * 64 + np * 32 + cb) = hv;
    }
  }
}

static int g_mhsa_force_long = 0;  // test knob: the blocked kernel at any length
void mhsa_set_force_long(int v) { g_mhsa_force_long = v != 0; }
static int g_mhsa_zsplit = 0;  // A/B knob: workgroups per (utterance, head) (0 = automatic)
void mhsa_set_zsplit(int v) { g_mhsa_zsplit = v; }
static int g_mhsa_vtr = 1;  // A/B knob: 1 (default) = V row-major in LDS + transposing reads, 0 = the V^T image (bit-identical)
void mhsa_set_vtr(int v) { g_mhsa_vtr = v != 0; }
static int g_mhsa_waves = 7;  // A/B knob: waves per workgroup of the one-pass kernel beyond 128 frames (4 or 7)
void mhsa_set_waves(int v) { g_mhsa_waves = v == 4 ? 4 : 7; }

template <class HT>
static void launch_mhsa_t(const void* qkv, void* out, int B, int T, int H, float scale, const int* lens, hipStream_t s) {
  typedef typename HT::T Tt;
  // up to 1.5 workgroups per CU (B x H <= 384) each head's query tiles are split over two workgroups, each staging K / V itself
  // (since the staging lost its V^T scatter the split pays through B = 24: teacher step 4.75 -> 4.72 ms at B = 16,
  // 6.26 -> 6.23 at B = 24, tools/diag_mhsa_vtr.py zsplit; rows do not depend on the split)
  dim3 grid(H, B, g_mhsa_zsplit > 0 ? g_mhsa_zsplit : ((long)H * B <= 384 && T > 64 ? 2 : 1)), blk(256);
  if (T > ATT_KEYS || g_mhsa_force_long)
    hipLaunchKernelGGL((mhsa_long_kernel<HT>), dim3(H, B, (T + 63) / 64), blk, 0, s, (const Tt*)qkv, (Tt*)out, T, H, scale, lens);
  else if (T <= 64 && g_mhsa_vtr)
    hipLaunchKernelGGL((mhsa_kernel<HT, 2, 4, false, true>), grid, blk, 0, s, (const Tt*)qkv, (Tt*)out, T, H, scale, lens, MhsaRing{});
  else if (T <= 64)
    hipLaunchKernelGGL((mhsa_kernel<HT, 2, 4>), grid, blk, 0, s, (const Tt*)qkv, (Tt*)out, T, H, scale, lens, MhsaRing{});
  else if (T <= 128 && g_mhsa_vtr)
    hipLaunchKernelGGL((mhsa_kernel<HT, 4, 4, false, true>), grid, blk, 0, s, (const Tt*)qkv, (Tt*)out, T, H, scale, lens, MhsaRing{});
  else if (T <= 128)
    hipLaunchKernelGGL((mhsa_kernel<HT, 4, 4>), grid, blk, 0, s, (const Tt*)qkv, (Tt*)out, T, H, scale, lens, MhsaRing{});
  else if (g_mhsa_waves == 4)
    hipLaunchKernelGGL((mhsa_kernel<HT, 7, 4>), grid, blk, 0, s, (const Tt*)qkv, (Tt*)out, T, H, scale, lens, MhsaRing{});
  else if (g_mhsa_vtr)
    hipLaunchKernelGGL((mhsa_kernel<HT, 7, 7, false, true>), grid, dim3(448), 0, s, (const Tt*)qkv, (Tt*)out, T, H, scale, lens, MhsaRing{});
  else
    hipLaunchKernelGGL((mhsa_kernel<HT, 7, 7>), grid, dim3(448), 0, s, (const Tt*)qkv, (Tt*)out, T, H, scale, lens, MhsaRing{});
}

// KV-cached streaming attention (see MhsaRing): ring (S, 256 slots, 3 H 64) operand type, out (S, 16, H 64).  The form
// (MhsaRingForm, afx_kernels.h) says where the valid counts and the query tile come from; the checks are made once, here.
#undef ring_qtile
static const char* ring_args(int S, int H, const MhsaRingForm& f, bool dtype_ok, MhsaRing* r) {
  if (S <= 0 || S > 65535 || H <= 0 || f.form < 1 || f.form > 3) return "mhsa_ring: bad shape";
  if (f.form < 3 && (f.q_tile < 0 || f.q_tile > 15)) return "mhsa_ring: bad shape";
  if (f.form == 1 ? !f.cnt : !f.tab) return "mhsa_ring: bad shape";
  if (!dtype_ok) return "mhsa_ring: half-precision operands only";
  *r = MhsaRing{};
  if (f.form < 3) r->q_tile = f.q_tile;
  for (int i = 0; f.form == 1 && i < 16; ++i) {
    if (f.cnt[i] < 0 || f.cnt[i] > 16) return "mhsa_ring: a group holds at most 16 frames";
    r->cnt[i] = (unsigned char)f.cnt[i];
  }
  return nullptr;
}
template <class HT>
static void launch_mhsa_ring_t(const void* ring, void* out, int S, int H, int form, const int* tab, const MhsaRing& r, hipStream_t s) {
  using Tt = typename HT::T;
  const dim3 grid(H, S, 1), blk(256);
  if (form == 1)
    hipLaunchKernelGGL((mhsa_kernel<HT, 8, 4, true, true>), grid, blk, 0, s, (const Tt*)ring, (Tt*)out, 256, H, 0.125f, nullptr, r);
  else if (form == 2)
    hipLaunchKernelGGL((mhsa_kernel<HT, 8, 4, 2, true>), grid, blk, 0, s, (const Tt*)ring, (Tt*)out, 256, H, 0.125f, tab, r);
  else
    hipLaunchKernelGGL((mhsa_kernel<HT, 8, 4, 3, true>), grid, blk, 0, s, (const Tt*)ring, (Tt*)out, 256, H, 0.125f, tab, r);
}
const char* launch_mhsa_ring(const void* ring, void* out, int S, int H, const MhsaRingForm& f, int dtype, hipStream_t s) {
  MhsaRing r;
  if (const char* m = ring_args(S, H, f, dtype == DT_FP16 || dtype == DT_BF16, &r)) return m;
  if (dtype == DT_BF16)
    launch_mhsa_ring_t<BF16>(ring, out, S, H, f.form, f.tab, r, s);
  else
    launch_mhsa_ring_t<FP16>(ring, out, S, H, f.form, f.tab, r, s);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

// fp32 rows in / out, products in split precision on the fp16 matrix pipe (the engine's "fp16x3"); T <= 224
const char* launch_mhsa_split(const float* qkv, float* out, int B, int T, int H, hipStream_t s, const int* lens, bool out_pairs, float out_scale) {
  if (T <= 0 || T > ATT_KEYS || B <= 0 || B > 65535 || H <= 0) return "mhsa_split: 1..224 frames";
  const float scale = 0.125f;
  dim3 grid(H, B, (long)H * B < 256 && T > 64 ? 2 : 1);
  const MhsaRing none = {};
  if (T <= 64) hipLaunchKernelGGL((mhsa_split_kernel<2, 4>), grid, dim3(256), 0, s, qkv, out, T, H, scale, lens, out_pairs ? 1 : 0, out_scale, none);
  else if (T <= 128) hipLaunchKernelGGL((mhsa_split_kernel<4, 4>), grid, dim3(256), 0, s, qkv, out, T, H, scale, lens, out_pairs ? 1 : 0, out_scale, none);
  else hipLaunchKernelGGL((mhsa_split_kernel<7, 7>), grid, dim3(448), 0, s, qkv, out, T, H, scale, lens, out_pairs ? 1 : 0, out_scale, none);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

// the ring forms in split precision: fp32 [q | k | v] slots in, fp32 rows (or pair-form rows) out -- (S, 16, H*64)
const char* launch_mhsa_ring_split(const float* ring, float* out, int S, int H, const MhsaRingForm& f, hipStream_t s, bool out_pairs,
                                   float out_scale) {
  MhsaRing r;
  if (const char* m = ring_args(S, H, f, true, &r)) return m;
  const dim3 grid(H, S, 1), blk(256);
  const int pairs = out_pairs ? 1 : 0;
  if (f.form == 1)
    hipLaunchKernelGGL((mhsa_split_kernel<8, 4, true>), grid, blk, 0, s, ring, out, 256, H, 0.125f, nullptr, pairs, out_scale, r);
  else if (f.form == 2)
    hipLaunchKernelGGL((mhsa_split_kernel<8, 4, 2>), grid, blk, 0, s, ring, out, 256, H, 0.125f, f.tab, pairs, out_scale, r);
  else
    hipLaunchKernelGGL((mhsa_split_kernel<8, 4, 3>), grid, blk, 0, s, ring, out, 256, H, 0.125f, f.tab, pairs, out_scale, r);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

const char* launch_mhsa(const void* qkv, void* out, int B, int T, int H, int dtype, hipStream_t s, const int* lens) {
  if (T <= 0 || B <= 0 || H <= 0) return "mhsa: bad shape";
  if (B > 65535 || (T + 63) / 64 > 65535) return "mhsa: batch / length beyond the launch grid";
  const float scale = 0.125f;  // 64^-0.5
  if (dtype == DT_FP32) {  // exact mode: fp32 VALU attention (afx_conformer.hip), q | k | v fp32 rows
    const float* f = (const float*)qkv;
    return launch_conf_attn(f, 3L * H * 64, f + H * 64, 3L * H * 64, nullptr, 0, B, T, H, 64, out, (long)H * 64, DT_FP32, s, lens, 0);
  }
  if (dtype == DT_BF16)
    launch_mhsa_t<BF16>(qkv, out, B, T, H, scale, lens, s);
  else
    launch_mhsa_t<FP16>(qkv, out, B, T, H, scale, lens, s);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

}  // namespace afx
