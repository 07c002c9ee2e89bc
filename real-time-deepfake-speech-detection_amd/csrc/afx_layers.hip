// Per-slot state kernels of the streaming layers (afx/_layer.py) for gfx950 and their C entry points (include/afx.h):
// cascade store / select / windows, verdict, evidence mark / copy, input quality, and provenance.
#include "../../include/afx.h"
#include "afx_common.h"
#include "afx_entry.h"

namespace afx {

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

extern "C" int afx_k_cascade_store(const float* x, int A, int hop, const int* hdr, float* hist, int S, int window,
                                   void* stream) {
  if (!x || !hdr || !hist) return fail("cascade_store: null argument");
  if (A <= 0 || A > 65535) return fail("cascade_store: 1 to 65535 rows");
  if (S <= 0 || window <= 0 || hop <= 0 || hop > window) return fail("cascade_store: a hop must be positive and fit the window");
  hipLaunchKernelGGL(cascade_store_kernel, dim3(min((hop + 1023) / 1024, 64), A), dim3(256), 0, (hipStream_t)stream, x, hdr, hist, S, window, hop);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail("%s", hipGetErrorString(e));
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

extern "C" int afx_k_cascade_select(const float* scores, int stride, const int* hdr, int A, int* wait, int* counts, int S,
                                    float threshold, int budget, int cooldown, int* sel, void* stream) {
  if (!scores || !hdr || !wait || !sel) return fail("cascade_select: null argument");
  if (stride < 1) return fail("cascade_select: a score stride of at least 1");
  if (A <= 0 || A > CASCADE_MAX_ROWS) return fail("cascade_select: 1 to 8192 rows");
  if (S <= 0) return fail("cascade_select: no slots");
  if (threshold != threshold) return fail("cascade_select: the threshold is NaN");
  if (budget < 1 || cooldown < 0) return fail("cascade_select: budget >= 1 and cooldown >= 0");
  const size_t lds = (size_t)max(A, 16) * sizeof(unsigned long long);
  hipLaunchKernelGGL(cascade_select_kernel, dim3(1), dim3(CASCADE_SELECT_THREADS), lds, (hipStream_t)stream, scores, stride, hdr, A, wait, counts,
                     S, threshold, budget, cooldown, sel);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail("%s", hipGetErrorString(e));
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

extern "C" int afx_k_cascade_windows(const float* hist, int S, int window, const int* hdr, int A, const int* sel, int budget,
                                     float* out, void* stream) {
  if (!hist || !hdr || !sel || !out) return fail("cascade_windows: null argument");
  if (S <= 0 || window <= 0 || A <= 0) return fail("cascade_windows: no slots, no window or no rows");
  if (budget < 1 || budget > 65535) return fail("cascade_windows: a budget of 1 to 65535 rows");
  hipLaunchKernelGGL(cascade_windows_kernel, dim3(min((window + 1023) / 1024, 64), budget), dim3(256), 0, (hipStream_t)stream, hist, S, window,
                     hdr, A, sel, budget, out);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail("%s", hipGetErrorString(e));
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

extern "C" int afx_k_verdict(const float* scores, int stride, const float* vscores, const int* hdr, int A, float* m, int* st,
                             int S, float alpha, float enter, float exit_, float verifier_enter, int confirm, int release,
                             int min_scores, int latch, int* log, int cap, void* stream) {
  if (!scores || !hdr || !m || !st || !log) return fail("verdict: null argument");
  if (stride < 1) return fail("verdict: a score stride of at least 1");
  if (A <= 0 || A > VERDICT_MAX_ROWS) return fail("verdict: 1 to 8192 rows");
  if (S <= 0) return fail("verdict: no slots");
  if (!(alpha > 0.f && alpha <= 1.f)) return fail("verdict: alpha in (0, 1]");
  if (enter != enter || exit_ != exit_) return fail("verdict: a threshold is NaN");
  if (verifier_enter != verifier_enter) return fail("verdict: the verifier threshold is NaN");
  if (exit_ < enter) return fail("verdict: exit below enter");
  if (confirm < 1 || release < 1 || min_scores < 1) return fail("verdict: confirm, release and min_scores of at least 1");
  if (latch != 0 && latch != 1) return fail("verdict: latch is 0 or 1");
  if (cap < 0) return fail("verdict: a negative log capacity");
  hipLaunchKernelGGL(verdict_kernel, dim3(1), dim3(VERDICT_THREADS), 0, (hipStream_t)stream, scores, stride, vscores, hdr, A, m, st, S, alpha, enter,
                     exit_, verifier_enter, confirm, release, min_scores, latch, log, cap);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail("%s", hipGetErrorString(e));
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

extern "C" int afx_k_evidence_mark(const int* hdr, int A, const int* vst, int S, int pre, int post, int* rec, int* left, int* claim,
                                   int* pool, int clips, int* counters, int* work, void* stream) {
  if (!hdr || !vst || !rec || !left || !claim || !pool || !counters || !work) return fail("evidence_mark: null argument");
  if (A <= 0 || A > EVIDENCE_MAX_ROWS) return fail("evidence_mark: 1 to 8192 rows");
  if (S <= 0) return fail("evidence_mark: no slots");
  if (pre < 0 || post < 0 || (long long)pre + post + 1 > 0x7fffffffll) return fail("evidence_mark: pre and post of 0 or more hops");
  if (clips < 1 || clips > EVIDENCE_MAX_CLIPS) return fail("evidence_mark: 1 to 8192 clips");
  hipLaunchKernelGGL(evidence_mark_kernel, dim3(1), dim3(EVIDENCE_THREADS), 0, (hipStream_t)stream, hdr, A, vst, S, pre, post, rec, left, claim, pool,
                     clips, counters, work);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail("%s", hipGetErrorString(e));
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

extern "C" int afx_k_evidence_copy(const float* x, const float* scores, int stride, const int* hdr, const int* work, int A, int hop,
                                   int pre, int post, float* hist, float* sring, int S, void* audio, float* cscores, int clips,
                                   int encoding, void* stream) {
  if (!x || !hdr || !work || !hist || !sring || !audio || !cscores) return fail("evidence_copy: null argument");
  if (scores && stride < 1) return fail("evidence_copy: a score stride of at least 1");
  if (A <= 0 || A > EVIDENCE_MAX_ROWS) return fail("evidence_copy: 1 to 8192 rows");
  if (S <= 0 || hop <= 0) return fail("evidence_copy: no slots or no hop");
  if (pre < 0 || post < 0 || ((long long)pre + 1) * hop > 0x7fffffffll || ((long long)pre + 1 + post) * hop > 0x7fffffffll)
    return fail("evidence_copy: pre and post of 0 or more hops, a ring and a clip below 2^31 samples");
  if (clips < 1 || clips > EVIDENCE_MAX_CLIPS) return fail("evidence_copy: 1 to 8192 clips");
  if (encoding != 0 && encoding != 1) return fail("evidence_copy: encoding 0 (fp32) or 1 (pcm16)");
  EvidenceCopyArgs a{};
  a.x = x; a.scores = scores; a.hdr = hdr; a.work = work; a.hist = hist; a.sring = sring; a.audio = audio; a.cscores = cscores;
  a.stride = scores ? stride : 0; a.A = A; a.hop = hop; a.pre = pre; a.post = post; a.S = S; a.clips = clips; a.pcm16 = encoding;
  hipLaunchKernelGGL(evidence_copy_kernel, dim3(min((hop + 1023) / 1024, 64), A), dim3(256), 0, (hipStream_t)stream, a);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail("%s", hipGetErrorString(e));
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

extern "C" int afx_k_quality(const float* x, long long stride, int A, int hop, const int* hdr, const float* scores, int sstride,
                             float clip, int clip_count, int flat_run, float e_quiet, float dc, int mask, int max_bad, int abstain,
                             unsigned char* ring, int W, int* state, int* totals, int S, int* meas, float* out, void* stream) {
  if (!x || !hdr || !ring || !state || !totals || !meas) return fail("quality: null argument");
  if (scores && (!out || sstride < 1)) return fail("quality: scores need an output and a stride of at least 1");
  if (A <= 0 || A > QUALITY_MAX_ROWS) return fail("quality: 1 to 8192 rows");
  if (hop <= 0 || hop > QUALITY_MAX_HOP) return fail("quality: a hop of 1 to 2^24 samples");
  if (stride < hop) return fail("quality: a row stride of at least the hop");
  if (S <= 0) return fail("quality: no slots");
  if (W < 1 || W > QUALITY_MAX_W) return fail("quality: a window of 1 to 1024 hops");
  if (!(clip > 0.f)) return fail("quality: clip above 0");
  if (clip_count < 1) return fail("quality: clip_count of at least 1");
  if (flat_run < 2) return fail("quality: flat_run of at least 2");
  if (!(e_quiet >= 0.f) || !(dc >= 0.f)) return fail("quality: the quiet and dc bounds are 0 or more");
  if (mask < 0 || mask > 31) return fail("quality: mask is 0 to 31");
  if (max_bad < 0) return fail("quality: max_bad of 0 or more");
  if (abstain != 0 && abstain != 1) return fail("quality: abstain is 0 or 1");
  QualityArgs a{};
  a.x = x; a.stride = stride; a.hdr = hdr; a.scores = reinterpret_cast<const int*>(scores); a.sstride = scores ? sstride : 0;
  a.ring = ring; a.state = state; a.totals = totals; a.meas = meas; a.out = scores ? reinterpret_cast<int*>(out) : nullptr;
  a.A = A; a.hop = hop; a.S = S; a.W = W;
  a.vec = reinterpret_cast<uintptr_t>(x) % 16 == 0 && stride % 4 == 0;
  a.clip = clip; a.e_quiet = e_quiet; a.dc = dc;
  a.clip_count = clip_count; a.flat_run = flat_run; a.mask = mask; a.max_bad = max_bad; a.abstain = abstain;
  hipLaunchKernelGGL(quality_kernel, dim3(A), dim3(256), 0, (hipStream_t)stream, a);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail("%s", hipGetErrorString(e));
}

// ---------------------------------------------------------------------------------
// Provenance (afx/provenance.py; the function is stated in include/afx.h afx_k_provenance): how many samples of each hop
// the jitter buffer made up, a ring of the last W hops' counts per slot, their sum, and the score passed on or replaced by
// NaN while the sum is above the limit.  All integers.  One thread per row, rows independent: the thread stores its hop's
// ring entry, recounts the window over at most W entries, and writes state, totals, meas and out.
// ---------------------------------------------------------------------------------
constexpr int PROV_MAX_ROWS = 8192;
constexpr int PROV_MAX_W = 1024;
constexpr int PROV_MAX_HOP = 1 << 24;

struct ProvArgs {
  const int* hdr;      // (A, 2): slot, hop index k
  const int* counts;   // (A,): the hop's synthetic samples
  const int* scores;   // the bits of the inner scores at a stride of `sstride` words, or nullptr
  int sstride;
  int* ring;           // (S, W): the count of hop j at (j - 1) mod W
  int* state;          // (S, 2): total, valid
  int* totals;         // (S, 3): hops, synthetic samples, withheld hops
  int* meas;           // (A, 3)
  int* out;            // (A,) bits of the scores passed on, or nullptr
  long long limit;
  int A, hop, S, W, abstain;
};

__global__ __launch_bounds__(256) void provenance_kernel(ProvArgs a) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= a.A) return;
  const int slot = a.hdr[2 * row], k = a.hdr[2 * row + 1], c = a.counts[row];
  const int sbits = a.scores ? a.scores[(long long)row * a.sstride] : 0;
  int* m = a.meas + 3ll * row;
  if (!(slot >= 0 && slot < a.S && k >= 1 && c >= 0 && c <= a.hop)) {
    m[0] = m[1] = m[2] = -1;
    if (a.out) a.out[row] = sbits;
    return;
  }
  int* rg = a.ring + (long long)slot * a.W;
  rg[(k - 1) % a.W] = c;
  const int n = min(k, a.W);  // hops k, k - 1, .., k - n + 1: never before the session's first
  long long sum = c;
  for (int i = 1; i < n; ++i) sum += rg[(k - 1 - i) % a.W];
  const int valid = sum <= a.limit, total = (int)min(sum, (long long)QUALITY_N_MAX);
  a.state[2ll * slot] = total;
  a.state[2ll * slot + 1] = valid;
  int* tot = a.totals + 3ll * slot;
  tot[0] = quality_sat_inc(tot[0], 1);
  tot[1] = quality_sat_inc(tot[1], c);
  tot[2] = quality_sat_inc(tot[2], 1 - valid);
  m[0] = c, m[1] = total, m[2] = valid;
  if (a.out) a.out[row] = valid || !a.abstain ? sbits : QUALITY_QNAN;
}

extern "C" int afx_k_provenance(const int* hdr, const int* counts, const float* scores, int sstride, int A, int hop, long long limit,
                                int abstain, int* ring, int W, int* state, int* totals, int S, int* meas, float* out, void* stream) {
  if (!hdr || !counts || !ring || !state || !totals || !meas) return fail("provenance: null argument");
  if (scores && (!out || sstride < 1)) return fail("provenance: scores need an output and a stride of at least 1");
  if (A <= 0 || A > PROV_MAX_ROWS) return fail("provenance: 1 to 8192 rows");
  if (hop <= 0 || hop > PROV_MAX_HOP) return fail("provenance: a hop of 1 to 2^24 samples");
  if (S <= 0) return fail("provenance: no slots");
  if (W < 1 || W > PROV_MAX_W) return fail("provenance: a window of 1 to 1024 hops");
  if (limit < 0 || limit > (long long)W * hop) return fail("provenance: a limit of 0 to W * hop samples");
  if (abstain != 0 && abstain != 1) return fail("provenance: abstain is 0 or 1");
  ProvArgs a{};
  a.hdr = hdr; a.counts = counts; a.scores = reinterpret_cast<const int*>(scores); a.sstride = scores ? sstride : 0;
  a.ring = ring; a.state = state; a.totals = totals; a.meas = meas; a.out = scores ? reinterpret_cast<int*>(out) : nullptr;
  a.limit = limit; a.A = A; a.hop = hop; a.S = S; a.W = W; a.abstain = abstain;
  hipLaunchKernelGGL(provenance_kernel, dim3((A + 255) / 256), dim3(256), 0, (hipStream_t)stream, a);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail("%s", hipGetErrorString(e));
}

}  // namespace afx
