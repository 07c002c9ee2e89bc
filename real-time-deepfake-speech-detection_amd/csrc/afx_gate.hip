// Speech-gate and talk-spurt kernels for gfx950 and their C entry points (include/afx.h): the three gate forms over their
// shared phases, the turn recurrence (streamed, closed, and scanned offline) and the turn clips.  Host side: afx/vad.py,
// turns.py.
#include "../../include/afx.h"
#include "afx_common.h"
#include "afx_entry.h"

namespace afx {

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

extern "C" int afx_k_gate(const float* x, int A, int n, const int* hdr, int frame, float e_floor, float ratio, float rise, int hang,
                          float* nf, int* h, float* ring, int S, int ring_len, int* kept, unsigned char* mask, void* stream) {
  KRET(gate_launch("gate", gate_args(x, n, hdr, frame, e_floor, ratio, rise, hang, nf, h, ring, S, ring_len, kept, mask), A,
                   [&](const GateArgs& g) { hipLaunchKernelGGL(gate_kernel, dim3(A), dim3(256), 0, (hipStream_t)stream, g); }));
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

extern "C" int afx_k_gate_la(const float* x, int A, int n, const int* hdr, int frame, float e_floor, float ratio, float rise,
                             int hang, int pre, float* nf, int* h, int* flags, float* line, float* ring, int* src, int S,
                             int ring_len, int* kept, unsigned char* mask, void* stream) {
  if (!flags || !line || !src) return fail("gate_la: null argument");
  if (frame > 0 && (S <= 0 || ring_len <= 0 || ring_len > (1 << 30) || ring_len % frame))
    return fail("gate_la: no slots, or a ring that is not whole frames (at most 2^30 samples)");
  if (pre < 1 || pre > 31) return fail("gate_la: 1 to 31 frames of pre-roll");
  GateLaArgs a{gate_args(x, n, hdr, frame, e_floor, ratio, rise, hang, nf, h, ring, S, ring_len, kept, mask), pre, flags, line, src};
  KRET(gate_launch("gate_la", a.g, A, [&](const GateArgs& g) {
    a.g = g;
    hipLaunchKernelGGL(gate_la_kernel, dim3(A), dim3(256), 0, (hipStream_t)stream, a);
  }));
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

extern "C" int afx_k_gate_tone(const float* x, int A, int n, const int* hdr, int frame, float e_floor, float ratio, float rise,
                               int hang, const float* coef, int K, float thr, int confirm, int hold, float* nf, int* h,
                               int* tone_state, float* ring, int S, int ring_len, int* kept, int* ntone, unsigned char* mask,
                               float* tsum, void* stream) {
  if (!coef || !tone_state) return fail("gate_tone: null argument");
  if (K < 1 || K > GATE_MAX_TONES) return fail("gate_tone: a bank of 1 to 16 frequencies");
  if (!(thr > 0.f && thr < INFINITY) || confirm < 1 || hold < 0)
    return fail("gate_tone: thr > 0 (finite), confirm >= 1 and hold >= 0");
  GateToneArgs a{gate_args(x, n, hdr, frame, e_floor, ratio, rise, hang, nf, h, ring, S, ring_len, kept, mask),
                 coef, tone_state, ntone, tsum, K, confirm, hold, thr};
  KRET(gate_launch("gate_tone", a.g, A, [&](const GateArgs& g) {
    a.g = g;
    hipLaunchKernelGGL(gate_tone_kernel, dim3(A), dim3(256), 0, (hipStream_t)stream, a);
  }));
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

extern "C" int afx_k_turn(const float* staging, int S, int ring_len, const unsigned char* mask, const int* hdr, int A, int F,
                          int frame, int min_frames, int max_frames, float* bufs, int* state, int* totals, int* done,
                          void* stream) {
  if (!staging || !mask || !hdr || !bufs || !state || !totals || !done) return fail("turn: null argument");
  if (A <= 0 || A > 65535) return fail("turn: 1 to 65535 rows");
  if (F < 1 || F > TURN_MAX_FRAMES) return fail("turn: 1 to 512 frames in a row");
  if (frame <= 0) return fail("turn: a frame is a positive number of samples");
  if (min_frames < F) return fail("turn: min_frames is at least the frames of a row (else a row could complete two turns)");
  if (min_frames > max_frames) return fail("turn: min_frames is at most max_frames");
  if (S <= 0 || (long long)F * frame > ring_len) return fail("turn: no slots, or a staging ring shorter than a row");
  if ((long long)max_frames * frame > 0x3fffffff) return fail("turn: a turn of more than 2^30 samples");
  TurnArgs a{staging, mask, hdr, bufs, state, totals, done, S, ring_len, F, frame, min_frames, max_frames,
             frame % 4 == 0 && ring_len % 4 == 0 && host_aligned16(staging) && host_aligned16(bufs)};
  hipLaunchKernelGGL(turn_kernel, dim3(A), dim3(256), 0, (hipStream_t)stream, a);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail("%s", hipGetErrorString(e));
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

extern "C" int afx_k_turn_collect(const float* bufs, int S, int max_frames, int frame, const int* rows, int R, float* out,
                                  void* stream) {
  if (!bufs || !rows || !out) return fail("turn_collect: null argument");
  if (S <= 0 || R <= 0 || R > 65535) return fail("turn_collect: 1 to 65535 rows");
  if (frame <= 0 || max_frames <= 0 || (long long)max_frames * frame > 0x3fffffff)
    return fail("turn_collect: a window of 1 to 2^30 samples in whole frames");
  const int W = max_frames * frame, vec = frame % 4 == 0 && host_aligned16(bufs) && host_aligned16(out);
  const int per = vec ? 1024 : 256;
  hipLaunchKernelGGL(turn_collect_kernel, dim3(min((W + per - 1) / per, 64), R), dim3(256), 0, (hipStream_t)stream, bufs, S, max_frames, frame,
                     rows, out, vec);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail("%s", hipGetErrorString(e));
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

extern "C" int afx_k_turn_close(const int* slots, int A, int S, int min_frames, int max_frames, int* state, int* totals, int* done,
                                void* stream) {
  if (!slots || !state || !totals || !done) return fail("turn_close: null argument");
  if (A <= 0 || A > 65535) return fail("turn_close: 1 to 65535 rows");
  if (S <= 0) return fail("turn_close: no slots");
  if (min_frames < 1) return fail("turn_close: min_frames is at least 1");
  if (min_frames > max_frames) return fail("turn_close: min_frames is at most max_frames");
  hipLaunchKernelGGL(turn_close_kernel, dim3((A + 255) / 256), dim3(256), 0, (hipStream_t)stream, slots, A, S, min_frames, max_frames, state, totals,
                     done);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail("%s", hipGetErrorString(e));
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

extern "C" int afx_k_turn_scan(const unsigned char* mask, const long long* offs, int A, int min_frames, int max_frames,
                               int close_end, int* table, int cap, int* row_base, int* totals, int* open, void* stream) {
  const hipStream_t s = (hipStream_t)stream;
  if (!mask || !offs || !table || !row_base || !totals || !open) return fail("turn_scan: null argument");
  if (A <= 0 || A > 65535) return fail("turn_scan: 1 to 65535 rows");
  if (min_frames < 1) return fail("turn_scan: min_frames is at least 1");
  if (min_frames > max_frames) return fail("turn_scan: min_frames is at most max_frames");
  if (cap < 0) return fail("turn_scan: a table of 0 or more rows");
  TurnScanArgs a{mask, offs, table, row_base, totals, open, A, min_frames, max_frames, close_end ? 1 : 0, cap};
  hipLaunchKernelGGL(turn_scan_kernel<false>, dim3(A), dim3(256), 0, s, a);
  hipLaunchKernelGGL(turn_scan_base_kernel, dim3(1), dim3(256), 0, s, row_base, A);
  if (cap > 0) hipLaunchKernelGGL(turn_scan_kernel<true>, dim3(A), dim3(256), 0, s, a);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail("%s", hipGetErrorString(e));
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

extern "C" int afx_k_turn_clips(const float* x, const long long* xoffs, int A, int frame, int max_frames, const int* table, int r0,
                                int R, float* out, void* stream) {
  if (!x || !xoffs || !table || !out) return fail("turn_clips: null argument");
  if (A <= 0) return fail("turn_clips: no recordings");
  if (r0 < 0 || R <= 0 || R > 65535) return fail("turn_clips: 1 to 65535 table rows from row r0 >= 0");
  if (frame <= 0 || max_frames <= 0 || (long long)max_frames * frame > 0x3fffffff)
    return fail("turn_clips: a window of 1 to 2^30 samples in whole frames");
  const int W = max_frames * frame, vec = frame % 4 == 0 && host_aligned16(out);
  const int per = vec ? 1024 : 256;
  hipLaunchKernelGGL(turn_clips_kernel, dim3(min((W + per - 1) / per, 64), R), dim3(256), 0, (hipStream_t)stream, x, xoffs, A, frame, max_frames,
                     table + 4 * (long long)r0, out, vec);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail("%s", hipGetErrorString(e));
}

// ---------------------------------------------------------------------------------
// Provenance counts behind a gate (afx/provenance.py; the functions are stated in include/afx.h afx_k_prov_compact /
// afx_k_prov_take): gsyn, (S, ring_frames) int32 parallel to the gate's pending ring in frames, holds per kept frame how
// many of its samples the jitter buffer made up.
//   compact: one workgroup per row of a gate launch.  Thread t owns the frames 2 t and 2 t + 1 (F <= 512); an exclusive scan
//            of bit 0 of their mask bytes -- inclusive over the wave by shuffle-up (w = 1 .. 32), the four waves' totals
//            through LDS -- gives each kept frame its rank among the kept ones, and its count goes to
//            gsyn[slot][(wpos / frame + rank) mod ring_frames]: the order in which gate_copy_kept compacts the samples;
//   take:    one wave per ready row sums the hop's `per` entries from head / frame on (lane l: l, l + 64, ...; a shuffle-down tree).
// ---------------------------------------------------------------------------------
constexpr int PROV_MAX_RING_FRAMES = 1 << 30;

// The exclusive scan of a workgroup of 256 threads: `mine` kept frames per thread -> the kept frames before this thread's.
// Inclusive over the wave by shuffle-up, the four waves' totals through s_wave (4 ints of LDS); every thread of the
// workgroup calls it (it passes one barrier).
__device__ __forceinline__ int prov_rank(int mine, int lane, int wave, int* s_wave) {
  int incl = mine;
  for (int w = 1; w < 64; w <<= 1) {
    const int o = __shfl_up(incl, w);
    if (lane >= w) incl += o;
  }
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  int rank = incl - mine;
  for (int w = 0; w < wave; ++w) rank += s_wave[w];
  return rank;
}

__global__ __launch_bounds__(256) void prov_compact_kernel(const int* __restrict__ counts, const unsigned char* __restrict__ mask,
                                                           const int* __restrict__ hdr, int F, int frame, int* __restrict__ gsyn,
                                                           int S, int ring_frames) {
  __shared__ int s_wave[4];
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int slot = hdr[2 * row], wpos = hdr[2 * row + 1], wposf = wpos / frame;  // (the gate launch's own header: samples)
  if (!(slot >= 0 && slot < S && wpos >= 0 && wpos % frame == 0 && wposf < ring_frames)) return;  // (the whole workgroup: no barrier is passed by some)
  int c[2], keep[2];
  bool bad = false;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int f = 2 * tid + j;
    const bool in = f < F;
    c[j] = in ? counts[(long long)row * F + f] : 0;
    keep[j] = in ? mask[(long long)row * F + f] & 1 : 0;
    bad |= c[j] < 0 || c[j] > frame;
  }
  if (__syncthreads_or(bad)) return;  // a count that is no frame's: the row is skipped whole
  int rank = prov_rank(keep[0] + keep[1], lane, wave, s_wave);
  int* dst = gsyn + (long long)slot * ring_frames;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (keep[j]) {
      const int at = wposf + rank;  // rank < F <= ring_frames: one wrap
      dst[at < ring_frames ? at : at - ring_frames] = c[j];
      ++rank;
    }
  }
}

extern "C" int afx_k_prov_compact(const int* counts, const unsigned char* mask, const int* hdr, int A, int F, int frame, int* gsyn,
                                  int S, int ring_frames, void* stream) {
  if (!counts || !mask || !hdr || !gsyn) return fail("prov_compact: null argument");
  if (A <= 0 || A > 65535) return fail("prov_compact: 1 to 65535 rows");
  if (S <= 0) return fail("prov_compact: no slots");
  if (F <= 0 || F > GATE_MAX_FRAMES) return fail("prov_compact: 1 to 512 frames a row");
  if (frame <= 0) return fail("prov_compact: a frame of at least 1 sample");
  if (ring_frames < F || ring_frames > PROV_MAX_RING_FRAMES) return fail("prov_compact: a ring of at least a row's frames, at most 2^30");
  hipLaunchKernelGGL(prov_compact_kernel, dim3(A), dim3(256), 0, (hipStream_t)stream, counts, mask, hdr, F, frame, gsyn, S,
                     ring_frames);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail("%s", hipGetErrorString(e));
}

__global__ __launch_bounds__(256) void prov_take_kernel(const int* __restrict__ gsyn, int S, int ring_frames,
                                                        const int* __restrict__ table, int R, int per, int frame, int* __restrict__ out) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= R) return;  // (the same for the 64 lanes of a wave; the kernel passes no barrier)
  const int slot = table[2 * row], head = table[2 * row + 1], headf = head / frame;  // (the pop's own table: samples)
  if (!(slot >= 0 && slot < S && head >= 0 && head % frame == 0 && headf < ring_frames)) {
    if (lane == 0) out[row] = -1;
    return;
  }
  const int* src = gsyn + (long long)slot * ring_frames;
  long long sum = 0;
  int neg = 0;
  for (int k = lane; k < per; k += 64) {
    const int at = headf + k;  // per <= ring_frames: one wrap
    const int v = src[at < ring_frames ? at : at - ring_frames];
    neg |= v < 0;
    sum += v;
  }
  for (int w = 32; w >= 1; w >>= 1) {
    sum += __shfl_down(sum, w);
    neg |= __shfl_down(neg, w);
  }
  if (lane == 0) out[row] = neg ? -1 : (int)min(sum, 0x7fffffffll);  // (a negative entry is no count: the row says so)
}

extern "C" int afx_k_prov_take(const int* gsyn, int S, int ring_frames, const int* table, int R, int per, int frame, int* out,
                               void* stream) {
  if (!gsyn || !table || !out) return fail("prov_take: null argument");
  if (S <= 0) return fail("prov_take: no slots");
  if (ring_frames <= 0 || ring_frames > PROV_MAX_RING_FRAMES) return fail("prov_take: a ring of 1 to 2^30 frames");
  if (R <= 0 || R > 65535 * 4) return fail("prov_take: 1 to 262140 rows");
  if (per <= 0 || per > ring_frames) return fail("prov_take: a hop's frames must fit the ring");
  if (frame <= 0) return fail("prov_take: a frame of at least 1 sample");
  hipLaunchKernelGGL(prov_take_kernel, dim3((R + 3) / 4), dim3(256), 0, (hipStream_t)stream, gsyn, S, ring_frames, table, R, per, frame, out);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail("%s", hipGetErrorString(e));
}

// ---------------------------------------------------------------------------------
// Provenance counts behind a look-ahead gate and through turns (afx/provenance.py; the functions are stated in
// include/afx.h afx_k_prov_compact_la / afx_k_prov_turn / afx_k_prov_turn_sum).  Integer copies and sums, beside the
// kernels they mirror:
//   compact_la: gate_la_kernel's emission for counts.  Mask entry j of a row is keep' of frame g = F - pre + j; the count of
//               an emitted frame comes out of gline (S, pre: delayed frame g at block g mod pre, parallel to `line`) for
//               j < pre and out of this row's counts[j - pre] otherwise.  One workgroup per row, thread t owns the entries
//               2 t and 2 t + 1; every gline read stands before prov_rank's barrier and every gline write (the row's last
//               min(pre, n_frames) counts: frame G enters the block frame G - pre leaves) behind it;
//   turn:       turn_kernel's plan for counts.  One wave per row: lane 0 replays the recurrence for open and n from the
//               slot's state (which it only reads: turn_kernel, launched next on the stream, moves it) and writes each kept
//               frame's destination among the slot's 2 x max_frames entries to LDS, the frames of a turn the row drops as
//               short taken out again (the next turn starts at the same place); then the lanes copy counts to bsyn;
//   turn_sum:   the count of a turn tiled to max_frames frames, q * sum(first m) + sum(first max_frames mod m); one wave per
//               row, the two partial sums through one shuffle-down tree.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void prov_compact_la_kernel(const int* __restrict__ counts, const unsigned char* __restrict__ mask,
                                                              const int* __restrict__ hdr, int n, int frame, int pre, int* gline,
                                                              int* __restrict__ gsyn, int S, int ring_frames) {
  __shared__ int s_wave[4];
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int slot = hdr[4 * row], wpos = hdr[4 * row + 1], F = hdr[4 * row + 2], wposf = wpos / frame;  // (afx_k_gate_la's header)
  if (!(slot >= 0 && slot < S && wpos >= 0 && wpos % frame == 0 && wposf < ring_frames && F >= 0 && F <= 0x7fffffff - n))
    return;  // (the whole workgroup: no barrier is passed by some)
  const int* cr = counts + (long long)row * n;
  int* gl = gline + (long long)slot * pre;
  int c[2], keep[2];
  bool bad = false;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int j = 2 * tid + k;
    const bool in = j < n;
    c[k] = in ? cr[j] : 0;
    bad |= c[k] < 0 || c[k] > frame;
  }
  if (__syncthreads_or(bad)) return;  // a count that is no frame's: the row is skipped whole
  int v[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int j = 2 * tid + k;
    const long long g = (long long)F - pre + j;  // the frame that leaves at step j
    keep[k] = j < n && g >= 0 && (mask[(long long)row * n + j] & 1);
    v[k] = !keep[k] ? 0 : j < pre ? gl[g % pre] : cr[j - pre];
  }
  int rank = prov_rank(keep[0] + keep[1], lane, wave, s_wave);  // (its barrier: every read of gline is done)
  int* dst = gsyn + (long long)slot * ring_frames;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int j = 2 * tid + k;
    if (keep[k]) {
      const int at = wposf + rank;  // rank < n <= ring_frames: one wrap
      dst[at < ring_frames ? at : at - ring_frames] = v[k];
      ++rank;
    }
    if (j < n && j >= n - pre) gl[(F + j) % pre] = c[k];  // (F + j < 2^31; the last min(pre, n) frames: distinct blocks)
  }
}

extern "C" int afx_k_prov_compact_la(const int* counts, const unsigned char* mask, const int* hdr, int A, int n_frames, int frame,
                                     int pre, int* gline, int* gsyn, int S, int ring_frames, void* stream) {
  if (!counts || !mask || !hdr || !gline || !gsyn) return fail("prov_compact_la: null argument");
  if (A <= 0 || A > 65535) return fail("prov_compact_la: 1 to 65535 rows");
  if (S <= 0) return fail("prov_compact_la: no slots");
  if (n_frames <= 0 || n_frames > GATE_MAX_FRAMES) return fail("prov_compact_la: 1 to 512 frames a row");
  if (frame <= 0) return fail("prov_compact_la: a frame of at least 1 sample");
  if (pre < 1 || pre > 31) return fail("prov_compact_la: 1 to 31 frames of pre-roll");
  if (ring_frames < n_frames || ring_frames > PROV_MAX_RING_FRAMES)
    return fail("prov_compact_la: a ring of at least a row's frames, at most 2^30");
  hipLaunchKernelGGL(prov_compact_la_kernel, dim3(A), dim3(256), 0, (hipStream_t)stream, counts, mask, hdr, n_frames, frame, pre,
                     gline, gsyn, S, ring_frames);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail("%s", hipGetErrorString(e));
}

__global__ __launch_bounds__(64) void prov_turn_kernel(const int* __restrict__ counts, const unsigned char* __restrict__ mask,
                                                       const int* __restrict__ hdr, int F, int frame, int min_frames, int max_frames,
                                                       const int* __restrict__ state, int* __restrict__ bsyn, int S) {
  __shared__ int s_plan[TURN_MAX_FRAMES];  // open * max_frames + n of a kept frame, -1: nothing to store
  const int row = blockIdx.x, lane = threadIdx.x;
  const int slot = hdr[3 * row], wpos = hdr[3 * row + 1], g0 = hdr[3 * row + 2];
  bool ok = slot >= 0 && slot < S && wpos >= 0 && g0 >= 0 && g0 <= 0x7fffffff - F;
  int open = 0, n = 0;
  if (ok) {
    open = state[3 * slot];
    n = state[3 * slot + 1];
    ok = (open == 0 || open == 1) && n >= 0 && n < max_frames;
  }
  if (!ok) return;  // (the whole wave)
  const int* cr = counts + (long long)row * F;
  bool bad = false;
  for (int j = lane; j < F; j += 64) bad |= cr[j] < 0 || cr[j] > frame;
  if (__syncthreads_or(bad)) return;  // a count that is no frame's: the row is skipped whole
  if (lane == 0) {
    const unsigned char* m = mask + (long long)row * F;
    int j0 = 0;  // the open turn's first frame in this row
    for (int j = 0; j < F; ++j) {
      if (m[j] & 1) {
        if (n == 0) j0 = j;
        s_plan[j] = open * max_frames + n;
        if (++n == max_frames) { open ^= 1; n = 0; }
      } else {
        s_plan[j] = -1;
        if (n > 0) {
          if (n >= min_frames) open ^= 1;
          else for (int k = j0; k < j; ++k) s_plan[k] = -1;
          n = 0;
        }
      }
    }
  }
  __syncthreads();
  int* dst = bsyn + (long long)slot * 2 * max_frames;
  for (int j = lane; j < F; j += 64) {
    const int p = s_plan[j];
    if (p >= 0) dst[p] = cr[j];
  }
}

extern "C" int afx_k_prov_turn(const int* counts, const unsigned char* mask, const int* hdr, int A, int F, int frame, int min_frames,
                               int max_frames, const int* state, int* bsyn, int S, void* stream) {
  if (!counts || !mask || !hdr || !state || !bsyn) return fail("prov_turn: null argument");
  if (A <= 0 || A > 65535) return fail("prov_turn: 1 to 65535 rows");
  if (F < 1 || F > TURN_MAX_FRAMES) return fail("prov_turn: 1 to 512 frames in a row");
  if (frame <= 0) return fail("prov_turn: a frame is a positive number of samples");
  if (min_frames < F) return fail("prov_turn: min_frames is at least the frames of a row (else a row could complete two turns)");
  if (min_frames > max_frames) return fail("prov_turn: min_frames is at most max_frames");
  if (S <= 0) return fail("prov_turn: no slots");
  if ((long long)max_frames * frame > 0x3fffffff) return fail("prov_turn: a turn of more than 2^30 samples");
  hipLaunchKernelGGL(prov_turn_kernel, dim3(A), dim3(64), 0, (hipStream_t)stream, counts, mask, hdr, F, frame, min_frames, max_frames,
                     state, bsyn, S);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail("%s", hipGetErrorString(e));
}

__global__ __launch_bounds__(256) void prov_turn_sum_kernel(const int* __restrict__ bsyn, int S, int max_frames,
                                                            const int* __restrict__ rows, int R, int* __restrict__ out) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= R) return;  // (the same for the 64 lanes of a wave; the kernel passes no barrier)
  const int slot = rows[3 * row], buf = rows[3 * row + 1], m = rows[3 * row + 2];
  if (slot < 0 || slot >= S || buf < 0 || buf > 1 || m < 1 || m > max_frames) {  // (turn_collect_kernel's guard)
    if (lane == 0) out[row] = -1;
    return;
  }
  const int* src = bsyn + ((long long)slot * 2 + buf) * max_frames;
  const int q = max_frames / m, rem = max_frames % m;
  long long whole = 0, part = 0;
  int neg = 0;
  for (int k = lane; k < m; k += 64) {
    const int v = src[k];
    neg |= v < 0;
    whole += v;
    if (k < rem) part += v;
  }
  for (int w = 32; w >= 1; w >>= 1) {
    whole += __shfl_down(whole, w);
    part += __shfl_down(part, w);
    neg |= __shfl_down(neg, w);
  }
  if (lane == 0) out[row] = neg ? -1 : (int)min(q * whole + part, 0x7fffffffll);  // (entries <= frame: at most the window)
}

extern "C" int afx_k_prov_turn_sum(const int* bsyn, int S, int max_frames, const int* rows, int R, int* out, void* stream) {
  if (!bsyn || !rows || !out) return fail("prov_turn_sum: null argument");
  if (S <= 0) return fail("prov_turn_sum: no slots");
  if (max_frames <= 0) return fail("prov_turn_sum: a window of at least 1 frame");
  if (R <= 0 || R > 65535 * 4) return fail("prov_turn_sum: 1 to 262140 rows");
  hipLaunchKernelGGL(prov_turn_sum_kernel, dim3((R + 3) / 4), dim3(256), 0, (hipStream_t)stream, bsyn, S, max_frames, rows, R, out);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail("%s", hipGetErrorString(e));
}

}  // namespace afx
