// Packet-front kernels for gfx950 and their C entry points (include/afx.h): polyphase resampling (offline and streamed),
// packet ingest in one or several formats, payload expand, and the jitter buffer's verbs.  They share one tile body,
// polyphase_tiles.  Host side: afx/resample.py, ingest.py, codecs.py, jitter.py.
#include "../../include/afx.h"
#include "afx_common.h"
#include "afx_entry.h"

namespace afx {

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

extern "C" int afx_k_resample(const float* x, const long long* in_offs, const long long* out_offs, int B, long long max_out,
                              const float* taps, int L, int M, int T, float* out, void* stream) {
  if (!in_offs || !out_offs) return fail("resample: null offsets");
  ResampleArgs a{};
  a.x = x; a.in_offs = in_offs; a.out_offs = out_offs; a.f = PolyFilter{taps, L, M, T, 0, 0}; a.out = out;
  KRET(launch_resample_any(false, a, B, max_out, (hipStream_t)stream));
}

extern "C" int afx_k_resample_stream(const float* x, int A, int n_in, float* hist, const int* slot, const float* taps, int L,
                                     int M, int T, float* out, void* stream) {
  const hipStream_t s = (hipStream_t)stream;
  if (!hist || !slot) return fail("resample_stream: null history or slot table");
  if (n_in <= 0 || M <= 0 || ((long long)n_in * L) % M != 0) return fail("resample_stream: n_in * L must be a multiple of M");
  if (T - 1 > 256) return fail("resample_stream: more than 256 carried samples");
  ResampleArgs a{};
  a.x = x; a.hist = hist; a.slot = slot; a.f = PolyFilter{taps, L, M, T, 0, 0}; a.n_in = n_in; a.out = out;
  const char* m = launch_resample_any(true, a, A, (long long)n_in * L / M, s);
  if (m || T == 1) KRET(m);
  hipLaunchKernelGGL(resample_hist_kernel, dim3(A), dim3(256), 0, s, x, n_in, slot, T - 1, hist);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail("%s", hipGetErrorString(e));
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

extern "C" int afx_k_ingest(const void* stage, long long stage_bytes, const int* hdr, int rows, int max_out, int enc,
                            const float* taps, int L, int M, int T, float* hist, float* ring, int S, int ring_len,
                            void* stream) {
  const hipStream_t s = (hipStream_t)stream;
  if (!stage || !hdr || !ring || stage_bytes <= 0) return fail("ingest: null staging buffer, header table or ring");
  if (enc < 0 || enc > 3) return fail("ingest: encoding 0 (pcm_f32le), 1 (pcm_s16le), 2 (mulaw) or 3 (alaw)");
  if (rows <= 0 || rows > 65535) return fail("ingest: 1 to 65535 rows");
  if (S <= 0 || ring_len <= 0 || max_out < 0 || max_out > ring_len) return fail("ingest: a row's outputs must fit its slot's ring");
  if (L <= 0 || M <= 0 || T <= 0) return fail("ingest: bad filter shape");
  const bool ident = taps == nullptr;
  if (ident && (L != 1 || M != 1 || T != 1)) return fail("ingest: no taps is the identity (L = M = T = 1)");
  if (!ident && T > 1 && !hist) return fail("ingest: null history");
  if (T - 1 > 256) return fail("ingest: more than 256 carried samples");
  IngestArgs a{};
  a.stage = (const unsigned char*)stage; a.stage_bytes = stage_bytes; a.hdr = hdr; a.hist = hist; a.ring = ring;
  a.f = PolyFilter{taps, L, M, T, 0, 0}; a.enc = enc; a.S = S; a.ring_len = ring_len;
  if (max_out > 0) {
    PolyGrid g;
    if (!poly_grid(a.f, ident, max_out, g)) return fail("ingest: input / output ratio above 12");
    const dim3 grid((unsigned)g.gx, rows);
    if (ident) hipLaunchKernelGGL((ingest_kernel<true, false>), grid, dim3(256), g.lds, s, a);
    else if (g.lds_taps) hipLaunchKernelGGL((ingest_kernel<false, true>), grid, dim3(256), g.lds, s, a);
    else hipLaunchKernelGGL((ingest_kernel<false, false>), grid, dim3(256), g.lds, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail("%s", hipGetErrorString(e));
  }
  if (T == 1) return 0;
  hipLaunchKernelGGL(ingest_hist_kernel, dim3(rows), dim3(256), 0, s, a);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail("%s", hipGetErrorString(e));
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

extern "C" int afx_k_ingest_mixed(const void* stage, long long stage_bytes, const int* hdr, int rows, const afx_ingest_format* formats,
                                  int n_formats, const int* max_out, float* hist, int Hs, float* ring, int S, int ring_len,
                                  void* stream) {
  const hipStream_t s = (hipStream_t)stream;
  if (n_formats < 1 || n_formats > ING_MAX_FORMATS) return fail("ingest_mixed: 1 to 16 formats");
  if (!formats || !max_out) return fail("ingest_mixed: null format table or output counts");
  IngestMixedArgs m{};
  PolyGrid g[ING_MAX_FORMATS];
  bool carried = false;
  for (int i = 0; i < n_formats; ++i) {
    const afx_ingest_format& d = formats[i];
    if (d.encoding < 0 || d.encoding > 3) return fail("ingest_mixed: encoding 0 (pcm_f32le), 1 (pcm_s16le), 2 (mulaw) or 3 (alaw)");
    if (d.L <= 0 || d.M <= 0 || d.T <= 0) return fail("ingest_mixed: bad filter shape");
    const bool ident = d.taps == nullptr;
    if (ident && (d.L != 1 || d.M != 1 || d.T != 1)) return fail("ingest_mixed: bad filter shape (no taps is the identity, L = M = T = 1)");
    if (d.T - 1 > 256) return fail("ingest_mixed: more than 256 carried samples");
    m.fmt[i].f = PolyFilter{d.taps, d.L, d.M, d.T, 0, 0};
    m.fmt[i].enc = d.encoding;
    if (!poly_grid(m.fmt[i].f, ident, max_out[i] > 0 ? max_out[i] : 0, g[i])) return fail("ingest_mixed: input / output ratio above 12");
    m.fmt[i].lds_taps = g[i].lds_taps;
    carried = carried || d.T > 1;
  }
  if (!stage || !hdr || !ring || stage_bytes <= 0) return fail("ingest_mixed: null staging buffer, header table or ring");
  if (rows <= 0 || rows > 65535) return fail("ingest_mixed: 1 to 65535 rows");
  if (S <= 0 || ring_len <= 0) return fail("ingest_mixed: a row's outputs must fit its slot's ring");
  long long gx = 0;
  size_t lds = 0;
  for (int i = 0; i < n_formats; ++i) {
    if (max_out[i] < 0 || max_out[i] > ring_len) return fail("ingest_mixed: a row's outputs must fit its slot's ring");
    if (formats[i].T - 1 > Hs) return fail("ingest_mixed: the history rows are narrower than a format's T - 1");
    if (max_out[i] > 0) {
      gx = g[i].gx > gx ? g[i].gx : gx;
      lds = g[i].lds > lds ? g[i].lds : lds;
    }
  }
  if (carried && !hist) return fail("ingest_mixed: null history");
  m.stage = (const unsigned char*)stage; m.stage_bytes = stage_bytes; m.hdr = hdr; m.hist = hist; m.ring = ring;
  m.S = S; m.ring_len = ring_len; m.Hs = Hs; m.nf = n_formats;
  if (gx > 0) {
    hipLaunchKernelGGL(ingest_mixed_kernel, dim3((unsigned)gx, rows), dim3(256), lds, s, m);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail("%s", hipGetErrorString(e));
  }
  if (!carried) return 0;
  hipLaunchKernelGGL(ingest_mixed_hist_kernel, dim3(rows), dim3(256), 0, s, m);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail("%s", hipGetErrorString(e));
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

extern "C" int afx_k_ingest_pop(const float* ring, int S, int ring_len, const int* table, int A, int hop, float* out,
                                void* stream) {
  if (!ring || !table || !out) return fail("ingest_pop: null argument");
  if (S <= 0 || A <= 0 || A > 65535) return fail("ingest_pop: 1 to 65535 rows");
  if (hop <= 0 || hop > ring_len) return fail("ingest_pop: a hop must fit the ring");
  hipLaunchKernelGGL(ingest_pop_kernel, dim3(min((hop + 255) / 256, 64), A), dim3(256), 0, (hipStream_t)stream, ring, S, ring_len, table, hop, out);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail("%s", hipGetErrorString(e));
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

extern "C" int afx_k_payload_expand(void* stage, long long stage_bytes, const int* hdr, int rows, int max_n, void* stream) {
  if (!stage || !hdr || stage_bytes <= 0) return fail("afx_k_payload_expand: null staging buffer or header table");
  if (rows <= 0 || rows > 65535) return fail("afx_k_payload_expand: 1 to 65535 rows");
  if (max_n < 0 || 4LL * max_n > stage_bytes) return fail("afx_k_payload_expand: a row's samples must fit the staging buffer");
  if (max_n == 0) return 0;  // no samples to write
  hipLaunchKernelGGL(payload_expand_kernel, dim3(min((max_n + 255) / 256, 64), rows), dim3(64), 0, (hipStream_t)stream, (unsigned char*)stage,
                     stage_bytes, hdr);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail("%s", hipGetErrorString(e));
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

// what every verb refuses of one entry of a rate table (ring_fit: how the entry point calls a J outside 1..Js)
static const char* jitter_rate_refusal(const char* who, const afx_jitter_rate& d, int Js, const char* ring_fit) {
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
static const char* jitter_launch(const char* who, JitterVerb verb, JitterRatesArgs m, const afx_jitter_rate* rates, int n_rates,
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
    const afx_jitter_rate& d = rates[i];
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
                                       int max_n, int enc, const afx_jitter_rate* rates, int n_rates, float* jring, int S, int Js,
                                       hipStream_t s) {
  JitterRatesArgs m{};
  m.stage = (const unsigned char*)stage; m.stage_bytes = stage_bytes; m.hdr = hdr; m.jring = jring; m.S = S; m.Js = Js;
  m.hdr_ints = hdr_ints; m.enc = enc; m.rated = hdr_ints == JIT_PLACE_RATES_HDR;
  return jitter_launch(who, JIT_PLACE, m, rates, n_rates, rows, &max_n, s);
}

static const char* jitter_conceal_launch(const char* who, float* jring, int S, int Js, const int* hdr, int hdr_ints, int rows, int max_n,
                                         const afx_jitter_rate* rates, int n_rates, int mode, hipStream_t s) {
  JitterRatesArgs m{};
  m.hdr = hdr; m.jring = jring; m.S = S; m.Js = Js; m.mode = mode;
  m.hdr_ints = hdr_ints; m.rated = hdr_ints == JIT_CONCEAL_RATES_HDR;
  return jitter_launch(who, JIT_CONCEAL, m, rates, n_rates, rows, &max_n, s);
}

static const char* jitter_release_launch(const char* who, const float* jring, int S, int Js, const int* hdr, bool rated, int rows,
                                         const afx_jitter_rate* rates, int n_rates, const int* max_out, float* ring, int ring_len,
                                         hipStream_t s) {
  JitterRatesArgs m{};
  m.hdr = hdr; m.jring = const_cast<float*>(jring); m.ring = ring; m.S = S; m.Js = Js; m.ring_len = ring_len;
  m.hdr_ints = JIT_RELEASE_HDR; m.rated = rated;
  return jitter_launch(who, JIT_RELEASE, m, rates, n_rates, rows, max_out, s);
}

static const char* jitter_noise_launch(const char* who, float* jring, int S, int Js, const int* hdr, int hdr_ints, int rows, int max_n,
                                       const afx_jitter_rate* rates, int n_rates, unsigned seed, const float* amp, hipStream_t s) {
  JitterRatesArgs m{};
  m.hdr = hdr; m.jring = jring; m.S = S; m.Js = Js; m.seed = seed; m.amp = amp;
  m.hdr_ints = hdr_ints; m.rated = hdr_ints == JIT_NOISE_RATES_HDR;
  return jitter_launch(who, JIT_NOISE, m, rates, n_rates, rows, &max_n, s);
}

// the one-rate entry points: a table of one entry built from their scalar arguments, Js = J, rows without a rate index
extern "C" int afx_k_jitter_place(const void* stage, long long stage_bytes, const int* hdr, int rows, int max_n, int enc,
                                  float* jring, int S, int J, void* stream) {
  const afx_jitter_rate one{nullptr, nullptr, 1, 1, 1, J, 0, 0};
  KRET(jitter_place_launch("jitter_place", stage, stage_bytes, hdr, JIT_PLACE_HDR, rows, max_n, enc, &one, 1, jring, S, J, (hipStream_t)stream));
}

extern "C" int afx_k_jitter_place_mixed(const void* stage, long long stage_bytes, const int* hdr, int rows, int max_n, float* jring,
                                        int S, int J, void* stream) {
  const afx_jitter_rate one{nullptr, nullptr, 1, 1, 1, J, 0, 0};
  KRET(jitter_place_launch("jitter_place_mixed", stage, stage_bytes, hdr, JIT_PLACE_MIXED_HDR, rows, max_n, 0, &one, 1,
                           jring, S, J, (hipStream_t)stream));
}

extern "C" int afx_k_jitter_conceal(float* jring, int S, int J, const int* hdr, int rows, int max_n, const float* fade, int P,
                                    int F, int mode, void* stream) {
  const afx_jitter_rate one{nullptr, fade, 1, 1, 1, J, P, F};
  KRET(jitter_conceal_launch("jitter_conceal", jring, S, J, hdr, JIT_CONCEAL_HDR, rows, max_n, &one, 1, mode, (hipStream_t)stream));
}

extern "C" int afx_k_jitter_release(const float* jring, int S, int J, const int* hdr, int rows, int max_out, const float* taps,
                                    int L, int M, int T, float* ring, int ring_len, void* stream) {
  const afx_jitter_rate one{taps, nullptr, L, M, T, J, 0, 0};
  KRET(jitter_release_launch("jitter_release", jring, S, J, hdr, false, rows, &one, 1, &max_out, ring, ring_len, (hipStream_t)stream));
}

extern "C" int afx_k_jitter_noise(float* jring, int S, int J, const int* hdr, int rows, int max_n, unsigned seed, const float* amp,
                                  void* stream) {
  const afx_jitter_rate one{nullptr, nullptr, 1, 1, 1, J, 0, 0};
  KRET(jitter_noise_launch("jitter_noise", jring, S, J, hdr, JIT_NOISE_HDR, rows, max_n, &one, 1, seed, amp, (hipStream_t)stream));
}

// the _rates entry points: the caller's table, rows that end in their rate index
extern "C" int afx_k_jitter_noise_rates(float* jring, int S, int Js, const int* hdr, int rows, int max_n, const afx_jitter_rate* rates,
                                        int n_rates, unsigned seed, const float* amp, void* stream) {
  KRET(jitter_noise_launch("jitter_noise_rates", jring, S, Js, hdr, JIT_NOISE_RATES_HDR, rows, max_n, rates, n_rates, seed, amp,
                           (hipStream_t)stream));
}

extern "C" int afx_k_jitter_place_rates(const void* stage, long long stage_bytes, const int* hdr, int rows, int max_n,
                                        const afx_jitter_rate* rates, int n_rates, float* jring, int S, int Js, void* stream) {
  KRET(jitter_place_launch("jitter_place_rates", stage, stage_bytes, hdr, JIT_PLACE_RATES_HDR, rows, max_n, 0, rates,
                           n_rates, jring, S, Js, (hipStream_t)stream));
}

extern "C" int afx_k_jitter_conceal_rates(float* jring, int S, int Js, const int* hdr, int rows, int max_n, const afx_jitter_rate* rates,
                                          int n_rates, int mode, void* stream) {
  KRET(jitter_conceal_launch("jitter_conceal_rates", jring, S, Js, hdr, JIT_CONCEAL_RATES_HDR, rows, max_n, rates, n_rates, mode,
                             (hipStream_t)stream));
}

extern "C" int afx_k_jitter_release_rates(const float* jring, int S, int Js, const int* hdr, int rows, const afx_jitter_rate* rates,
                                          int n_rates, const int* max_out, float* ring, int ring_len, void* stream) {
  KRET(jitter_release_launch("jitter_release_rates", jring, S, Js, hdr, true, rows, rates, n_rates, max_out, ring, ring_len, (hipStream_t)stream));
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
                                     int rows, int max_n, const afx_jitter_rate* rates, const afx_jitter_lags* lags, int n_rates,
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
    const afx_jitter_rate& d = rates[i];
    const afx_jitter_lags& g = lags[i];
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

extern "C" int afx_k_jitter_pitch(const float* jring, int S, int J, const int* hdr, int rows, int Pmin, int Pmax, int Wc, int P0,
                                  int* period, void* stream) {
  const afx_jitter_rate one{nullptr, nullptr, 1, 1, 1, J, 0, 0};
  const afx_jitter_lags lag{Pmin, Pmax, Wc, P0, 0};
  KRET(jitter_lag_launch("jitter_pitch", true, const_cast<float*>(jring), S, J, hdr, JIT_PITCH_HDR, false, rows, 0, &one, &lag, 1, period,
                         (hipStream_t)stream));
}

extern "C" int afx_k_jitter_pitch_rates(const float* jring, int S, int Js, const int* hdr, int rows, const afx_jitter_rate* rates,
                                        const afx_jitter_lags* lags, int n_rates, int* period, void* stream) {
  KRET(jitter_lag_launch("jitter_pitch_rates", true, const_cast<float*>(jring), S, Js, hdr, JIT_PITCH_RATES_HDR, true, rows, 0, rates, lags,
                         n_rates, period, (hipStream_t)stream));
}

extern "C" int afx_k_jitter_conceal_period(float* jring, int S, int J, const int* hdr, int rows, int max_n, const float* gain,
                                           const int* period, int Pmin, int Pmax, int P0, int Hd, int F, void* stream) {
  const afx_jitter_rate one{nullptr, gain, 1, 1, 1, J, P0, F};
  const afx_jitter_lags lag{Pmin, Pmax, 1, P0, Hd};  // (the synthesis reads no correlation window)
  KRET(jitter_lag_launch("jitter_conceal_period", false, jring, S, J, hdr, JIT_CONCEAL_HDR, false, rows, max_n, &one, &lag, 1,
                         const_cast<int*>(period), (hipStream_t)stream));
}

extern "C" int afx_k_jitter_conceal_period_rates(float* jring, int S, int Js, const int* hdr, int rows, int max_n,
                                                 const afx_jitter_rate* rates, const afx_jitter_lags* lags, int n_rates, const int* period,
                                                 void* stream) {
  KRET(jitter_lag_launch("jitter_conceal_period_rates", false, jring, S, Js, hdr, JIT_CONCEAL_RATES_HDR, true, rows, max_n, rates, lags,
                         n_rates, const_cast<int*>(period), (hipStream_t)stream));
}

// ---------------------------------------------------------------------------------
// Provenance marks of a jitter front (afx/provenance.py; the functions are stated in include/afx.h afx_k_prov_spans /
// afx_k_prov_frames): psyn, (S, ring_len) bytes parallel to the pending ring, holds 1 where the 16 kHz sample at that ring
// position was made up by the jitter buffer (loss concealment or comfort noise) and 0 where it was received.
//   spans:  rows of (slot, wpos, n, value) fill psyn[slot][(wpos + k) mod ring_len] = value, k < n; the host cuts every
//           release's output range into such runs, so the rows of a launch write disjoint ranges.  A range is at most two
//           linear pieces (before and after the wrap); each piece is written as its unaligned head and tail bytes and the
//           aligned dwords between them, a grid of (tile, row) striding over both;
//   frames: one wave per (row, frame) of the hops a pop takes: lane l counts the bytes l, l + 64, ... of the frame that are
//           not 0 (byte loads, the wrap taken per byte), a shuffle-down tree folds the 64 partials (w = 32 .. 1), lane 0
//           stores the count.  Integers: any order gives the same number.
// ---------------------------------------------------------------------------------
constexpr int PROV_MAX_RING = 1 << 30;  // bytes of a psyn row: positions and sums of two of them stay below 2^31

// p[0 .. n) = v for the threads t0, t0 + step, ... of a row's grid
__device__ __forceinline__ void prov_fill(unsigned char* p, int n, unsigned char v, int t0, int step) {
  if (n <= 0) return;
  const int head = min(n, (int)((4u - (unsigned)((unsigned long long)p & 3ull)) & 3u));
  const int words = (n - head) >> 2, tail = n - head - 4 * words;
  for (int i = t0; i < head; i += step) p[i] = v;
  unsigned* w = reinterpret_cast<unsigned*>(p + head);
  const unsigned vv = 0x01010101u * v;
  for (int q = t0; q < words; q += step) w[q] = vv;
  for (int i = t0; i < tail; i += step) p[head + 4 * words + i] = v;
}

__global__ __launch_bounds__(256) void prov_spans_kernel(unsigned char* __restrict__ psyn, int S, int ring_len,
                                                         const int* __restrict__ rows) {
  const int* r = rows + 4 * blockIdx.y;
  const int slot = r[0], wpos = r[1], n = r[2], value = r[3];
  if (!(slot >= 0 && slot < S && wpos >= 0 && wpos < ring_len && n >= 0 && n <= ring_len && (value == 0 || value == 1))) return;
  unsigned char* row = psyn + (long long)slot * ring_len;
  const int t0 = blockIdx.x * blockDim.x + threadIdx.x, step = gridDim.x * blockDim.x;
  const int n1 = min(n, ring_len - wpos);  // up to the ring's end; the rest from column 0
  prov_fill(row + wpos, n1, (unsigned char)value, t0, step);
  prov_fill(row, n - n1, (unsigned char)value, t0, step);
}

extern "C" int afx_k_prov_spans(unsigned char* psyn, int S, int ring_len, const int* rows, int R, int max_n, void* stream) {
  if (!psyn || !rows) return fail("prov_spans: null argument");
  if (S <= 0) return fail("prov_spans: no slots");
  if (ring_len <= 0 || ring_len > PROV_MAX_RING) return fail("prov_spans: a ring of 1 to 2^30 bytes");
  if (R <= 0 || R > 65535) return fail("prov_spans: 1 to 65535 rows");
  if (max_n < 0 || max_n > ring_len) return fail("prov_spans: the longest row is 0 to ring_len bytes");
  hipLaunchKernelGGL(prov_spans_kernel, dim3(max(min((max_n + 1023) / 1024, 64), 1), R), dim3(256), 0, (hipStream_t)stream, psyn, S,
                     ring_len, rows);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail("%s", hipGetErrorString(e));
}

__global__ __launch_bounds__(256) void prov_frames_kernel(const unsigned char* __restrict__ psyn, int S, int ring_len,
                                                          const int* __restrict__ table, int hop, int frame, int* __restrict__ out) {
  const int row = blockIdx.y, F = hop / frame;
  const int f = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (f >= F) return;  // (the same for the 64 lanes of a wave; the kernel passes no barrier)
  const int slot = table[2 * row], head = table[2 * row + 1];
  int* o = out + (long long)row * F + f;
  if (!(slot >= 0 && slot < S && head >= 0 && head < ring_len)) {
    if (lane == 0) *o = -1;
    return;
  }
  const unsigned char* src = psyn + (long long)slot * ring_len;
  const long long at = (long long)head + (long long)f * frame;  // < 2 ring_len: hop <= ring_len
  const int w0 = (int)(at < ring_len ? at : at - ring_len);
  int c = 0;
  for (int k = lane; k < frame; k += 64) {
    const int w = w0 + k;  // frame <= ring_len: one wrap
    c += src[w < ring_len ? w : w - ring_len] != 0;
  }
  for (int w = 32; w >= 1; w >>= 1) c += __shfl_down(c, w);
  if (lane == 0) *o = c;
}

extern "C" int afx_k_prov_frames(const unsigned char* psyn, int S, int ring_len, const int* table, int R, int hop, int frame,
                                 int* out, void* stream) {
  if (!psyn || !table || !out) return fail("prov_frames: null argument");
  if (S <= 0) return fail("prov_frames: no slots");
  if (ring_len <= 0 || ring_len > PROV_MAX_RING) return fail("prov_frames: a ring of 1 to 2^30 bytes");
  if (R <= 0 || R > 65535) return fail("prov_frames: 1 to 65535 rows");
  if (hop <= 0 || hop > ring_len) return fail("prov_frames: a hop must fit the ring");
  if (frame <= 0 || hop % frame != 0) return fail("prov_frames: a hop is a whole number of frames");
  hipLaunchKernelGGL(prov_frames_kernel, dim3((hop / frame + 3) / 4, R), dim3(256), 0, (hipStream_t)stream, psyn, S, ring_len, table,
                     hop, frame, out);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail("%s", hipGetErrorString(e));
}

}  // namespace afx
