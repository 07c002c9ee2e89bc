"""Jitter buffer of the streaming scorers: timestamped packets from a lossy network in, scores out.

``afx.ingest.PacketScorer`` takes each packet as the next bytes of its slot's stream.  Packets that crossed a network
carry an RTP timestamp and arrive late, twice, out of order or not at all.  ``JitterScorer`` wraps any of the three
streaming scorers and does per slot, on the GPU, what a telephony endpoint does: reorder, suppress duplicates, play out
behind a fixed depth and conceal what is missing -- and states what a slot's scores are a function of.

The contract.  Each slot has a played-out stream E, indexed in input-rate samples from the session's origin, the timestamp
of the first packet accepted after ``reset``.  Per slot the host keeps ``hi`` (the largest end index received), ``next``
(the playout point: everything below it has been released; it never moves back) and the received intervals in
[next, hi) -- from timestamps and sizes alone, so nothing is read back from the device.

  placement    a packet with timestamp t and n samples covers [t, t + n).  Samples below ``next`` are late: dropped and
               counted.  Samples already covered are duplicates: the first arrival wins, per sample, the rest are counted.
               All others are placed.  A packet may straddle any of these boundaries.
  playout      after a ``feed`` each named slot releases [next, max(next, hi - depth)); ``flush`` releases up to ``hi``;
               ``advance(slots, upto)`` up to a given index (clock-driven playout of a stream that went quiet).
  concealment  a released index that was received has its exact fp32 decode.  A released gap [a, b) is, with d = i - a,
               "zero":   E[i] = 0
               "repeat": E[i] = fade[d] * E[a - P + (d mod P)] for d < F, 0 for d >= F, E[<0] = 0
               with P the repeat period and F the fade length in input samples and fade[d] = fp32(1 - d/F) (computed in
               float64).  The source [a - P, a) may itself hold concealed samples: E is a stream.  Received samples are
               never modified.
  scores       the slot's j-th score is, bit for bit, score j of a fresh inner scorer pushed ``Resampler(input_rate)(E)``
               hop by hop, emitted by the call in which the last input sample it needs was released.

So with no loss and every packet arriving before the playout point passes its start, E is the sent stream and the scores
are an in-order lossless ``PacketScorer``'s whatever the permutation, the cuts and the duplicates; and ``depth = 0`` with
in-order input is ``PacketScorer``, call by call.

Device side (csrc/afx_packets.hip): one decoded reorder ring per slot, (S, J) fp32, index i at column i mod J.
``afx_k_jitter_place`` decodes all placed sub-ranges of a feed in one launch, ``afx_k_jitter_conceal`` writes released gaps
into the ring (one launch per rank of gap within a slot, so a gap whose source overlaps an earlier gap reads concealed
data), ``afx_k_jitter_release`` resamples released samples from the ring into the pending 16 kHz ring with the offline
kernel's inputs, taps and fma order, and ``afx_k_ingest_pop`` hands whole hops to the inner scorer's non-paced ``push``.
Sizing: with lookback = max(T - 1, P + F) (the filter history and a fading gap's source) and W = J - lookback >= depth,
every launch of a round whose playout point is ``cur`` touches only indices in [cur - lookback, cur + W): J consecutive
indices, no two on one column.  A forward jump or a packet longer than W is worked off in rounds (place what fits, conceal,
release, pop), so device memory does not depend on it.  A call is one pinned upload (payloads, then every table).

Sessions: ``export_slots`` adds ``jitter_pending`` / ``jitter_fill`` (pending 16 kHz samples), ``jitter_ring`` (the ring
columns [next - lookback, hi) left-aligned), ``jitter_book`` (origin, started, next, hi, open gap, largest start, last
sequence number, SSRC), ``jitter_stats`` and ``jitter_intervals`` ((n, K, 2), -1 padded) to the inner state, with meta
``jitter`` (format), ``jitter_depth``, ``jitter_conceal``, ``jitter_period``, ``jitter_fade``, ``input_rate`` and ``resampler``.

Several encodings at one clock rate: the reorder ring is decoded, so a session does not depend on how a packet was encoded.
``JitterScorer(scorer, input_rate, ("mulaw", "alaw"), ...)`` lists the encodings its packets may come in: ``feed`` takes one
per packet (``encodings``; default: the first listed), ``feed_rtp`` any datagram whose payload type maps to a listed one, and
a stream may change between them from packet to packet.  The place rows then carry their encoding
(``afx_k_jitter_place_mixed``: the same kernel with the encoding read per row).  State layout and contract are unchanged.

Every slot its own clock rate: ``MixedJitterScorer(scorer, formats, depth_ms, ...)`` takes 1 to 16 (input_rate, encoding)
pairs; a slot's rate is chosen at ``reset(slots, rates)``.  Per rate r, in that rate's samples: depth_r = depth_ms * r //
1000, P_r = r // 100 (``period_ms`` given: max(1, period_ms * r // 1000)), F_r = 3 P_r (``fade_ms`` given: fade_ms * r //
1000); P_r = F_r = 0 with conceal="zero".  The contract: take a slot s at rate r, whatever the other slots' rates.  Its
scores, hop counts per call, ``stats()``, ``samples_in``, ``buffered`` and ``pending`` are, bit for bit and call for call,
those of ``JitterScorer(inner, r, encodings_at_r, depth_r, conceal, period=P_r, fade=F_r, max_pending, ts_bits)`` fed the
slot's own packets in the same calls: the inner scorer runs on ``Resampler(r)(E_s)`` with E_s the played-out stream defined
above.  No new arithmetic: the rate is a per-row value of the same three launches (``afx_k_jitter_place_rates`` /
``_conceal_rates`` / ``_release_rates``: the row's last int names its rate, the workgroup runs its verb's one row body
with that rate's J, P, F, fade table and filter; a one-rate launch is the same kernel with a table of one entry), so every
value comes from the same decoder, the same single fp32 multiply and the same taps and ascending-j fma chain as in a
one-rate launch, and the host plans each slot with its own L, M, J, W, F and depth: ``JitterScorer`` is the scorer whose
table of rates has one entry and whose every slot is at index 0.  Sizing: per rate JitterScorer's lookback_r =
max(T_r - 1, P_r + F_r), W_r = depth_r + ceil(hop * M_r / L_r) + 1, J_r = lookback_r + W_r; one ring (S, Js), Js = max J_r;
a slot at rate r uses the columns [0, J_r) of its row with modulus J_r and never a column at or beyond J_r, so the
invariant above holds per slot with its own J_r.  A mixed state has ``jitter_ring`` (n, widest lookback_r + depth_r), zeros beyond a session's own columns,
``jitter_rate`` ((n,) int64) and ``jitter_params`` ((n, 3) int64: depth, period, fade), and the meta ``jitter``,
``jitter_conceal``, ``resampler`` and ``jitter_mixed``; a plain JitterScorer's state imports where its rate is listed and
its parameters are that rate's.  Out of scope: a rate change without a reset, per-slot depth within one rate, per-slot
conceal modes.

Expanded codecs: a listed encoding may be one of ``afx.codecs.CODECS`` (``dvi4``, ``pcm_s16be``, ``pcm_s24be``, ``pcm_u8``), and
packets of different codecs may share a call (``encodings=``).  DVI4 fits the decoded reorder ring because each RTP packet
carries its own predictor state: a packet decodes on its own, whatever was lost or reordered, and one with timestamp t and B
bytes covers [t, t + 2 (B - 4)).  Right after payload validation such a packet becomes a pcm_f32le block of the call's decoded
zone (``afx.ingest`` module docstring): placement, holes, late / duplicate trimming and the rounds run as above on encoding 0
with 4 bytes per sample -- a sub-range that starts k samples into a packet is read at its block + 4 k -- behind one "expand"
op (``afx_k_payload_expand``) issued before the call's first place.  A call without such a packet plans and issues what it
did.  ``feed_rtp`` knows RFC 3551's static audio types (``afx.rtp.STATIC_AUDIO_FORMATS``: 5, 6, 16, 17 are DVI4 at 8, 16,
11.025 and 22.05 kHz, 11 is mono L16 at 44.1 kHz in network byte order) and takes one without ``payload_types`` when its
(rate, encoding) is listed at the slot's rate.  The ring is decoded, so a state does not say which codec fed it.  Out of
scope: stereo (PT 10) / channel de-interleave, G.722 / G.726 and other codecs whose state runs across packets.

Pitch-period concealment: ``conceal="pitch_sync"`` repeats the last PITCH PERIOD of E instead of a fixed 10 ms, as telephone
endpoints do (G.711 Appendix I and its descendants), so a gap in voiced speech carries no discontinuity at every wrap and no
100 Hz buzz.  All lengths in the slot's input-rate samples at rate r; module constants, engineering defaults, NOT tuned:
Pmin = r // 400 (2.5 ms, 400 Hz), Pmax = 3 r // 200 (15 ms, 66.7 Hz), Wc = r // 50 (the 20 ms correlation window)
(``pitch_lags``); P0 = r // 100, the fallback period (``period``, inside [Pmin, Pmax]); Hd = r // 100, 10 ms at full level
(``hold``); F = r // 20, the fade (``fade``); G = Hd + F; Lh = Pmax + Wc.  A released gap with origin a (the start of the maximal
run of non-received indices, as above) is, with d = i - a:
      q[j]  = quant(E[j]) for j in [a - Lh, a);  E[<0] = 0
      quant(x): y = x * 32768f (one fp32 multiply);  NaN -> 0;  else clamp(rint(y) (ties to even), -32768, 32767), an integer
      for p in Pmin..Pmax:
          c(p) = sum_{j in [a-Wc, a)} q[j] * q[j-p]                       (exact integers, < 2**43)
          e(p) = sum_{j in [a-Wc, a)} q[j-p]**2
          s(p) = (float64(c) * float64(c)) / float64(e)   if c > 0 and e > 0, else "no candidate"
      p* = the p with the largest s(p), the smallest such p on a tie;  P0 if there is no candidate
      E[a + d] = gain[d] * E[a - p* + (d mod p*)]  for d < G  (one fp32 multiply of two stored fp32 values);  0 for d >= G
      gain[d] = 1 for d < Hd;  fp32(1 - (d - Hd)/F) for Hd <= d < G   (computed in float64, rounded once)
The search is exact integer arithmetic, so any summation order gives the same numbers; the floating-point operations are one
fp32 multiply per written sample and, per lag, one float64 multiply and one float64 divide, each correctly rounded.  p* is fixed
when index a is released, from E as it stands then (it may hold an earlier gap's concealed samples or comfort noise), and holds
for the whole gap, however many calls and rounds release it.  Received samples are never modified; with comfort noise the loss
part before a mark is concealed by this rule, counted from the run's origin; ``stats()`` counts what it counts.
``quantize``, ``pitch_reference(history, rate)`` and ``gain_table(hold, fade)`` are the statement in numpy.
Device side: two verbs of their own (``afx_k_jitter_conceal`` keeps refusing any mode but 0 and 1).  ``afx_k_jitter_pitch`` (rows
of (slot, a mod J [, rate index]): one workgroup per gap whose origin is released) writes p* to ``jperiod`` ((S,) int32, device
state: the host never learns it, nothing is read back); ``afx_k_jitter_conceal_period`` is the conceal launch with the row's
period read from there (a stored value outside [Pmin, Pmax] reads as P0).  Plan: per rank, a ("pitch", rows, Lh) op with the
rank's d_lo = 0 rows, if any, directly before the rank's ("conceal", ...) op, so the estimate obeys the order of the gaps too.
Sizing: lookback = max(T - 1, Pmax + max(Wc, G)) -- Pmax + Wc is the search history when a is released, Pmax + G the source of
a gap's last audible sample -- with W and J as above and the same J-window invariant; an all-zero row is rebased past G.
Sessions: ``reset`` zeroes the slot's period; ``export_slots`` adds ``jitter_pitch`` ((n,) int64: the period of the slot's open
loss gap, 0 where none is open; masked on the device) and the meta ``jitter_hold`` and ``jitter_lags`` ((Pmin, Pmax, Wc)), in this
mode only; ``import_slots`` refuses a gap younger than G whose period is outside [Pmin, Pmax]; states of different modes refuse
each other.  ``MixedJitterScorer(..., hold_ms=)``: per rate as ``period_ms`` / ``fade_ms``; its ``jitter_params`` gain a fourth
column, the hold.  A scorer built with "zero" or "repeat" plans, launches and exports exactly what it did.  Out of scope:
overlap-add into released or received samples (the contract forbids modifying them), multi-period repetition for long gaps,
voicing decisions, per-slot modes.

Silence suppression (DTX) and comfort noise (RFC 3389): a sender with VAD on stops sending in a pause and says so with a
CN packet: from this timestamp on there is silence, and the background noise is this many dB below overload.  A scorer built
with ``comfort_noise=ComfortNoise(seed)`` plays noise of that level where a scorer without it conceals a loss.  Opt-in: a
scorer without it is in every respect the scorer described above.
  marks        per slot the host keeps silence marks (t, level): t an index of E (unwrapped like a packet timestamp), level
               in 0..127.  A mark covers no samples and moves neither ``hi`` nor the origin.  ``silence(slots, timestamps,
               levels)`` registers them (``feed_rtp``: a datagram of payload type 13, or of a type mapped to "cn"; level =
               payload[0] & 0x7f; the spectral bytes after it are read past: a receiver of model order 0).  A mark for a slot
               without a session, or with t < ``next`` at the call that brings it, is dropped and counted (``marks_late``); of
               two marks of a slot at one t the first arrival wins.
  concealment  gains one case.  Let i be a released index that was not received and g the start of the maximal run of
               non-received indices that contains i (the gap origin a above).  If the slot holds a mark with g <= t <= i,
               E[i] is comfort noise at the level l of the mark with the largest such t; otherwise E[i] is concealed as
               above with d = i - g.  So a gap [g, b) with a mark at t is loss in [g, t) -- the lost last packet of a talk
               spurt is still concealed -- and noise in [t, b), whatever d is; a later mark in the run changes the level
               from its own t on.  E[i] is fixed by the call that releases i, from the intervals and marks accepted up to
               and including that call.  Received samples are never modified; the source [a - P, a) of a later loss gap may
               hold noise.  Marks inside received intervals govern nothing; marks are dropped as the playout point passes.
  noise        i is a 64-bit index, all integer arithmetic is mod 2**32, the one floating-point operation is one fp32 multiply:
                   x = lo32(i) * 0x9E3779B9 + hi32(i) * 0x85EBCA6B + seed
                   x ^= x >> 16;  x *= 0x7FEB352D;  x ^= x >> 15;  x *= 0x846CA68B;  x ^= x >> 16
                   k = int32(x) >> 8                     (arithmetic: -2**23 <= k < 2**23, exactly an fp32 number)
                   E[i] = amp[l] * fp32(k),   amp[l] = fp32(sqrt(3) * 10**(-l/20) / 2**23)   (float64, rounded once)
               uniform white noise of RMS 10**(-l/20) of the decoders' full scale (RFC 3389's -dBov, a full-scale square
               wave being 0 dBov).  It depends on (seed, i, l) only: not on the slot, the cut into calls or a session move.
               Nothing is clipped.  ``ComfortNoise.samples`` / ``.ints`` / ``.amp`` are the statement in numpy.
Device side: a fourth verb, ``afx_k_jitter_noise`` (``_noise_rates``): rows of (slot, column, n, lo32(i0), hi32(i0), level),
the launch shape of place.  A released gap is split at its governing marks into loss parts (conceal rows, ranked as before)
and noise parts (noise rows).  Per round: place, ONE noise launch, the conceal ranks, release, pop -- so a loss gap whose
source is this round's noise reads it.  Noise is written inside the released range only, as concealed samples are: ring
sizing and the J-window invariant are unchanged.  ``advance`` beyond ``hi`` continues a silence in force as noise.
``stats()`` adds ``comfort`` (noise samples released), ``marks`` (accepted) and ``marks_late``; ``concealed`` then counts
loss-concealed samples only.  ``export_slots`` adds ``jitter_cn_marks`` ((n, K, 2) int64, -1 padded: the marks at t >= next),
``jitter_cn_open`` ((n,) int64: the level in force for the open gap, -1 none), ``jitter_cn_stats`` ((n, 3) int64) and the
meta ``jitter_cn`` (the seed).  A state without them imports into a comfort-noise scorer with no marks; a state with them is
refused by a scorer without ``ComfortNoise`` or of another seed.  ``feed_rtp(..., ignore_types=(101,))`` parses and
SSRC-checks datagrams of those payload types (RFC 4733 telephone-events) and drops them.  Out of scope: spectral shaping from
the CN payload, inferring silence from the RTP marker bit, G.729 / AMR SID frames, per-slot seeds, noise in loss gaps,
generating CN on a sending side.

Provenance (``afx.provenance``): over a chain that holds a ``ProvenanceScorer``, the scorer keeps ``psyn``, (S, ring_len)
bytes parallel to the pending ring: 1 where the 16 kHz sample was made up here (a loss part in any mode, or comfort noise).
Per round the plan gains one ("spans", rows, longest row) op directly after the round's release (more than one where the
round has more than 65 535 span rows), rows of (slot, wpos, n, value) that partition every release row's output range
(``afx_k_prov_spans``), and every pop one ``afx_k_prov_frames`` launch
whose counts are noted to what stands below.  ``export_slots`` adds ``jitter_syn`` (laid out as ``jitter_pending``, uint8).
Over a chain without the layer nothing of this exists: plans, launches, state keys and bits are what they were.
"""
import ctypes as C
from itertools import repeat

import numpy as np
import torch

from . import rtp
from ._layer import StreamState, _on, check_pending, export_pending, import_pending, peel, rows_on, wrap
from ._lib import JitterLags, JitterRate, call_on, check, lib, ptr
from .codecs import CODECS
from .provenance import discover
from .ingest import (_MAX_SAMPLES, _SAMPLE, _UNIT, ENCODINGS, MAX_FORMATS, _at, _encoding, _format, device_encoding, expand_zone, layout,
                     with_expand)
from .resample import FILTER_ID, Resampler
from .streaming import _Front

JITTER_FORMAT = 1  # layout of the jitter part of a StreamState: import_slots refuses any other
CONCEAL = ("zero", "repeat", "pitch_sync")  # "zero" and "repeat": the library's mode numbers 0, 1; "pitch_sync": verbs of its own
PLACE_HDR, CONCEAL_HDR, RELEASE_HDR = 4, 4, 8  # int32 per row of the three tables (include/afx.h)
PITCH_HDR, PITCH_RATES_HDR = 2, 3  # afx_k_jitter_pitch / _pitch_rates: slot, column of the gap origin [, rate index]
PLACE_MIXED_HDR = 5  # afx_k_jitter_place_mixed: a place row, then its encoding's number
PLACE_RATES_HDR, CONCEAL_RATES_HDR = 6, 5  # afx_k_jitter_place_rates / _conceal_rates: the row, then its rate's index
STATS = ("received", "late", "duplicate", "concealed", "out_of_order")
_STATE_KEYS = ("jitter_pending", "jitter_fill", "jitter_ring", "jitter_book", "jitter_stats", "jitter_intervals")
_BOOK = ("origin", "started", "next", "hi", "gap", "max_start", "max_seq", "ssrc")  # jitter_book columns
_COUNTERS = ("received", "late", "dup", "concealed", "ooo")  # jitter_stats columns (STATS order)
_BPS = np.array([_SAMPLE[e].itemsize for e in ENCODINGS], dtype=np.int64)  # bytes per sample by encoding number
_NAMES = ENCODINGS + CODECS  # what a packet may come in, by the host's number: an encoding's own, then 4 + the codec's
_HOST_NUMBER = {e: i for i, e in enumerate(_NAMES)}
_HOST_UNIT = np.array([_UNIT[e] for e in _NAMES], dtype=np.int64)  # bytes a packet is a whole number of, by host number
NOISE_HDR, NOISE_RATES_HDR = 6, 7  # afx_k_jitter_noise / _noise_rates: slot, column, n, lo32(i0), hi32(i0), level [, rate index]
SPANS_MAX_ROWS = 65535  # rows of one afx_k_prov_spans launch (include/afx.h): a round's span rows go in ops of at most this many
CN_STATS = ("comfort", "marks", "marks_late")  # what stats() adds with a ComfortNoise
_CN_KEYS = ("jitter_cn_marks", "jitter_cn_open", "jitter_cn_stats")  # what export_slots adds with a ComfortNoise
_CN_COUNTERS = ("comfort", "nmarks", "marks_late")  # jitter_cn_stats columns (CN_STATS order)
_M32 = 0xFFFFFFFF


def _nonneg_int(v, name, least=0):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < least:
        raise ValueError(f"{name}: an integer >= {least}, got {v!r}")
    return int(v)


def pitch_lags(rate):
    """(Pmin, Pmax, Wc) of "pitch_sync" at ``rate`` Hz, in samples: the lags of 400 Hz and 66.7 Hz and the 20 ms correlation
    window (module docstring; engineering defaults, not tuned)."""
    return rate // 400, 3 * rate // 200, rate // 50


def quantize(x):
    """``quant`` of "pitch_sync" (module docstring): fp32 samples -> the integers the pitch search runs on (int64 array)."""
    with np.errstate(invalid="ignore", over="ignore"):
        y = np.asarray(x, dtype=np.float32) * np.float32(32768)
        return np.where(np.isnan(y), np.float32(0), np.clip(np.rint(y), -32768, 32767)).astype(np.int64)


def gain_table(hold, fade):
    """``gain`` of "pitch_sync": (hold + fade,) fp32, 1 for ``hold`` samples, then fp32(1 - (d - hold)/fade)."""
    d = np.arange(hold + fade, dtype=np.float64)
    return np.where(d < hold, 1.0, 1.0 - (d - hold) / max(fade, 1)).astype(np.float32)


def pitch_reference(history, rate, period=None):
    """p* of "pitch_sync" for a gap at ``rate`` Hz whose origin follows ``history`` (fp32, the samples of E before it, oldest
    first; the last Pmax + Wc are read, zeros stand before a shorter one); ``period``: the fallback P0, default rate // 100.
    Operation by operation what ``afx_k_jitter_pitch`` does: exact integer sums, one float64 multiply and divide per lag."""
    Pmin, Pmax, Wc = pitch_lags(rate)
    best, best_s, Lh = rate // 100 if period is None else period, None, Pmax + Wc
    h = quantize(np.asarray(history, dtype=np.float32).reshape(-1)[-Lh:])
    q = np.zeros(Lh, dtype=np.int64)
    q[Lh - h.size:] = h
    for p in range(Pmin, Pmax + 1):
        ref = q[Pmax - p:Lh - p]
        c, e = int(q[Pmax:] @ ref), int(ref @ ref)
        if c > 0 and e > 0:
            s = np.float64(c) * np.float64(c) / np.float64(e)
            if best_s is None or s > best_s:  # (ascending p: of equal scores the smallest lag stays)
                best, best_s = p, s
    return best


class ComfortNoise:
    """The comfort noise of a jitter scorer (module docstring, "noise"): ``seed`` is an integer in [0, 2**32), one for the
    whole scorer.  ``amp``: (128,) fp32, the amplitude of each level.  ``ints(i0, n)``: k of the indices i0 .. i0 + n - 1
    (int32); ``samples(i0, n, level)``: E of those indices at ``level`` (fp32), operation by operation what the kernel does."""

    def __init__(self, seed=0):
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed <= _M32:
            raise ValueError(f"seed: an integer in 0..2**32 - 1, got {seed!r}")
        self.seed = int(seed)
        self.amp = (np.sqrt(3.0) * 10.0 ** (-np.arange(128, dtype=np.float64) / 20.0) / 2.0 ** 23).astype(np.float32)

    def ints(self, i0, n):
        if not 0 <= i0 < 1 << 63 or n < 0:
            raise ValueError("ints: 0 <= i0 < 2**63 and n >= 0")
        i, m = np.uint64(i0) + np.arange(int(n), dtype=np.uint64), np.uint64(_M32)
        x = ((i & m) * np.uint64(0x9E3779B9) + (i >> np.uint64(32)) * np.uint64(0x85EBCA6B) + np.uint64(self.seed)) & m
        x ^= x >> np.uint64(16)
        x = (x * np.uint64(0x7FEB352D)) & m
        x ^= x >> np.uint64(15)
        x = (x * np.uint64(0x846CA68B)) & m
        x ^= x >> np.uint64(16)
        return x.astype(np.uint32).view(np.int32) >> 8

    def samples(self, i0, n, level):
        if isinstance(level, bool) or not isinstance(level, (int, np.integer)) or not 0 <= level <= 127:
            raise ValueError(f"level: an integer in 0..127, got {level!r}")
        return self.amp[level] * self.ints(i0, n).astype(np.float32)


class _Book:
    """The host's bookkeeping of every slot (int64 arrays over S) and, for the slots that currently have holes, their
    received intervals (``holes``: slot -> sorted disjoint [start, end) lists inside [next, hi)).  A slot that is not in
    ``holes`` has received exactly [next, hi).  Comfort noise: ``cn_open`` (the level in force for the open gap, -1 none),
    its counters and ``marks`` (slot -> the pending silence marks [t, level], sorted by t, every t >= next)."""

    _ARRAYS = _BOOK + _COUNTERS + _CN_COUNTERS + ("cn_open", "head", "fill")

    def __init__(self, S):
        for f in self._ARRAYS:
            setattr(self, f, np.zeros(S, dtype=np.int64))
        for f in ("gap", "max_seq", "ssrc", "cn_open"):
            getattr(self, f)[:] = -1
        self.holey = np.zeros(S, dtype=bool)
        self.holes, self.marks = {}, {}

    def copy(self):
        b = _Book.__new__(_Book)
        for f in self._ARRAYS + ("holey",):
            setattr(b, f, getattr(self, f).copy())
        b.holes, b.marks = dict(self.holes), dict(self.marks)  # (the lists are replaced, never edited in place)
        return b

    def clear(self, idx):
        for f in self._ARRAYS:
            getattr(self, f)[idx] = 0
        for f in ("gap", "max_seq", "ssrc", "cn_open"):
            getattr(self, f)[idx] = -1
        self.holey[idx] = False
        for s in idx:
            self.holes.pop(s, None)
            self.marks.pop(s, None)

    def intervals(self, s):
        """The received intervals of slot s in [next, hi)."""
        if self.holey[s]:
            return self.holes[s]
        return [[int(self.next[s]), int(self.hi[s])]] if self.hi[s] > self.next[s] else []

    def set_intervals(self, s, ivs):
        nxt, hi = int(self.next[s]), int(self.hi[s])
        if (not ivs and nxt == hi) or (len(ivs) == 1 and ivs[0][0] == nxt and ivs[0][1] == hi):
            self.holey[s] = False
            self.holes.pop(s, None)
        else:
            self.holey[s] = True
            self.holes[s] = ivs


def _subtract(lo, hi, ivs):
    """[lo, hi) minus the sorted disjoint intervals ``ivs`` -> list of [start, end)."""
    out = []
    for a, b in ivs:
        if b <= lo:
            continue
        if a >= hi:
            break
        if a > lo:
            out.append([lo, a])
        lo = max(lo, b)
        if lo >= hi:
            break
    if lo < hi:
        out.append([lo, hi])
    return out


def _merge(ivs, new):
    """Sorted disjoint ``ivs`` plus the intervals ``new`` (disjoint from them), touching intervals joined."""
    out = []
    for a, b in sorted(ivs + new):
        if out and a <= out[-1][1]:
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
    return out


class Plan:
    """What a call will do: ``ops`` (the launches, in order: ("place" | "noise" | "pitch" | "conceal" | "release" | "spans", int32 rows, largest row) and
    ("pop", (A, 2) table, slots)), ``counts`` (hops per named row) and ``book`` (the bookkeeping after it)."""

    def __init__(self, ops, slots, counts, book):
        self.ops, self.slots, self.counts, self.book = ops, slots, counts, book


class JitterScorer(_Front):
    """``scorer`` (a SlidingWindowScorer, IncrementalScorer or KVCachedScorer) fed timestamped packets at ``input_rate`` Hz
    in ``encoding`` (``afx.ingest.ENCODINGS`` or ``afx.codecs.CODECS``; a tuple of them: any of these per packet, the first the default); see the
    module docstring for the contract.

    ``depth``: the playout delay in input samples (60 ms is common; 0 is legal; the filter's ``delay`` comes on top of it).
    ``conceal``: "repeat", "zero" or "pitch_sync".  ``period``: the repeat period P in input samples, default 10 ms (input_rate // 100).  ``fade``: the fade length F in
    input samples, default 3 P (30 ms).  With "pitch_sync" (module docstring) ``period`` is the fallback P0 of the pitch search
    and must lie in its lags, ``fade`` defaults to 50 ms and ``hold`` (10 ms; this mode only) is the full-level part before the
    fade; ``lags`` = (Pmin, Pmax) and ``corr`` = Wc are the search's range and window.
    ``max_pending``: the whole hops a slot may buffer between ``feed(..., score=False)``
    and ``drain``.  ``ts_bits``: 32 (default) unwraps each timestamp to the value nearest the slot's ``hi``, so a stream
    crossing 2**32 is seamless; None takes absolute indices.  ``comfort_noise``: a ``ComfortNoise``, for calls with silence
    suppression (module docstring); None: silence marks and RTP payload type 13 are refused.

    Every jitter scorer owns a table of its rates (``_size``) and each slot's index into it; this one's table has one entry,
    every slot is at index 0, and the entry's values go by the names below (``depth``, ``period``, ``J`` ...)."""

    _WORK = "decoded, concealed, resampled"
    _rated = False  # (MixedJitterScorer: the rows of a plan carry their slot's rate index)

    def __init__(self, scorer, input_rate, encoding, depth, conceal="repeat", period=None, fade=None, max_pending=4, ts_bits=32,
                 comfort_noise=None, hold=None):
        if isinstance(encoding, str):
            self.encodings, self._mixed = (_encoding(encoding),), False
        else:
            if not isinstance(encoding, (tuple, list)) or not encoding:
                raise ValueError(f"encoding {encoding!r}: one of {ENCODINGS + CODECS}, or a tuple of them")
            self.encodings, self._mixed = tuple(_encoding(e) for e in encoding), True
            if len(set(self.encodings)) != len(self.encodings):
                raise ValueError("encoding: an encoding is listed twice")
        self.encoding = self.encodings[0]
        self.depth = _nonneg_int(depth, "depth")
        max_pending = self._checked(conceal, max_pending, ts_bits, comfort_noise)
        super().__init__(scorer, input_rate)
        self.period = self.fade_len = 0  # (no part of the "zero" function: not recorded in a state either)
        self.hold, self.lags, self.corr = 0, (0, 0), 0  # (parts of the "pitch_sync" function only)
        if hold is not None and conceal != "pitch_sync":
            raise ValueError(f'hold: a part of conceal="pitch_sync", not of {conceal!r}')
        if conceal == "repeat":
            self.period = _nonneg_int(self.input_rate // 100 if period is None else period, "period", 1)
            self.fade_len = _nonneg_int(3 * self.period if fade is None else fade, "fade")
        elif conceal == "pitch_sync":
            Pmin, Pmax, self.corr = pitch_lags(self.input_rate)
            self.lags = (Pmin, Pmax)
            self.period = _nonneg_int(self.input_rate // 100 if period is None else period, "period", 1)
            if not Pmin <= self.period <= Pmax:
                raise ValueError(f"period {self.period}: the fallback of the pitch search lies in its lags, {Pmin}..{Pmax}")
            self.fade_len = _nonneg_int(self.input_rate // 20 if fade is None else fade, "fade")
            self.hold = _nonneg_int(self.input_rate // 100 if hold is None else hold, "hold")
        self._size([self.rs], [self.encodings], [self.depth], [self.period], [self.fade_len], max_pending, [self.hold])
        self.L, self.M, self.J, self.fade = self.rs.L, self.rs.M, self.Js, self._fades[0]
        self.lookback, self.W = int(self._rlookback[0]), int(self._rW[0])

    def _checked(self, conceal, max_pending, ts_bits, comfort_noise=None):
        """The constructor arguments every jitter scorer takes, checked: sets ``conceal``, ``ts_bits`` and ``cn`` -> max_pending."""
        if comfort_noise is not None and not isinstance(comfort_noise, ComfortNoise):
            raise ValueError("comfort_noise: a ComfortNoise, or None")
        self.cn = comfort_noise
        if conceal not in CONCEAL:
            raise ValueError(f"conceal {conceal!r}: one of {CONCEAL}")
        max_pending = _nonneg_int(max_pending, "max_pending", 1)
        if ts_bits is not None and (isinstance(ts_bits, bool) or not isinstance(ts_bits, (int, np.integer)) or not 8 <= ts_bits <= 48):
            raise ValueError("ts_bits: None (absolute indices) or the width of the timestamp counter, 8..48")
        self.conceal, self.ts_bits = conceal, None if ts_bits is None else int(ts_bits)
        return max_pending

    def _size(self, rs, encs_at, depth, P, F, max_pending, hold):
        """The table of this scorer's rates, one entry per Resampler of ``rs`` (int64 arrays over the rates; ``depth``, ``P``,
        ``F`` and ``hold`` in each rate's own samples, ``encs_at`` the encodings listed at each), the device buffers sized from
        it, the host table the ``_rates`` launches take, and every slot at rate index 0."""
        scorer = self.scorer
        arr = lambda v: np.array(v, dtype=np.int64)
        self._rs, self._encs_at = list(rs), [tuple(e) for e in encs_at]
        self._rates = tuple(x.rate for x in rs)  # in Hz, in the order first listed
        self._renc = arr([device_encoding(e[0])[0] for e in self._encs_at])  # the default encoding's number, as place reads it
        self._rdefault = arr([_HOST_NUMBER[e[0]] for e in self._encs_at])  # the default encoding's host number
        self._listed = np.zeros((len(rs), len(_NAMES) + 1), dtype=bool)  # [rate index, host number]: listed at that rate
        for i, e in enumerate(self._encs_at):
            self._listed[i, [_HOST_NUMBER[v] for v in e]] = True
        self._rrate, self._rL, self._rM = arr(self._rates), arr([x.L for x in rs]), arr([x.M for x in rs])
        self._rdepth, self._rP, self._rF = arr(depth), arr(P), arr(F)
        # the sizing invariant (module docstring), per rate: J = lookback + W, W >= depth; the slack beyond depth is what a
        # round can place and release at once (one hop of input: an ordinary packet never takes a second round)
        pitch = self.conceal == "pitch_sync"
        self._rHd = arr(hold)
        self._rG = self._rHd + self._rF  # the samples of a gap that are not zeros (F itself outside "pitch_sync")
        self._rPmin, self._rPmax, self._rWc = (arr(v) for v in zip(*(pitch_lags(r) if pitch else (0, 0, 0) for r in self._rates)))
        # the source a gap reads until it is silent; "pitch_sync": also the search history Pmax + Wc when its origin is released
        back = self._rPmax + np.maximum(self._rWc, self._rG) if pitch else self._rP + self._rF
        self._rlookback = np.maximum(arr([0 if x.identity else x.T - 1 for x in rs]), back)
        self._rW = self._rdepth + -(-scorer.hop * self._rM // self._rL) + 1
        self._rJ = self._rlookback + self._rW
        self._rdelay = np.array([x.delay for x in rs], dtype=np.float64)
        self.Js = int(self._rJ.max())
        if self.Js >= _MAX_SAMPLES:
            raise ValueError("depth + period + fade: less than 2**30 samples")
        self._new_ring(max_pending)
        # provenance (afx.provenance): with a provenance layer below, (whom the counts of a pop are noted to, the samples of a
        # frame of those counts, whether that is an attached gate) and the marks of the pending ring's samples; else None
        self._prov = discover(self)
        if self._prov is not None:
            self.psyn = torch.zeros(scorer.S, self.ring_len, dtype=torch.uint8, device=scorer.device)
        self.jring = torch.zeros(scorer.S, self.Js, dtype=torch.float32, device=scorer.device)
        if pitch:  # one gain table per rate, and the period of each slot's open gap (device state: written by the estimate)
            self._fades = [torch.from_numpy(gain_table(int(h), int(f)) if h + f else np.ones(1, np.float32)).to(scorer.device)
                           for h, f in zip(self._rHd, self._rF)]
            self.jperiod = torch.zeros(scorer.S, dtype=torch.int32, device=scorer.device)
            self._lags = (JitterLags * len(rs))(*(JitterLags(*(int(a[i]) for a in (self._rPmin, self._rPmax, self._rWc, self._rP, self._rHd)))
                                                  for i in range(len(rs))))
        else:
            self._fades = [_fade_table(int(f), scorer.device) for f in self._rF]  # one device table per rate
        self._amp = None if self.cn is None else torch.from_numpy(self.cn.amp).to(scorer.device)
        self._table = (JitterRate * len(rs))()  # (pointers: the tensors above)
        for i, (t, x) in enumerate(zip(self._table, rs)):
            t.taps = None if x.identity else x.taps.data_ptr()
            t.fade = self._fades[i].data_ptr()
            t.L, t.M, t.T = x.L, x.M, 1 if x.identity else x.T
            t.J, t.P, t.F = int(self._rJ[i]), int(self._rP[i]), int(self._rF[i])
        self._b = _Book(scorer.S)
        self._rate_of = np.zeros(scorer.S, dtype=np.int64)  # rate index of each slot (host)

    # ---- properties ----------------------------------------------------------------------------------------------------
    @property
    def _fill(self):
        return self._b.fill

    @property
    def samples_in(self):
        """(S,) int64: each slot's playout point ``next``: the input-rate samples of E released since its last ``reset``."""
        return torch.from_numpy(self._b.next.copy())

    @property
    def buffered(self):
        """(S,) int64: hi - next, the span of input samples each slot's reorder ring holds back."""
        return torch.from_numpy(self._b.hi - self._b.next)

    def stats(self):
        """Per-slot int64 counters since each slot's reset: ``received`` (samples placed), ``late`` (samples below the
        playout point on arrival), ``duplicate`` (samples already covered), ``concealed`` (released gap samples) and
        ``out_of_order`` (packets that arrived behind an earlier one: by sequence number in ``feed_rtp``, by timestamp in
        ``feed``).  With a ``ComfortNoise``: also ``comfort`` (released noise samples), ``marks`` (silence marks accepted)
        and ``marks_late`` (marks dropped: no session yet, or below the playout point); ``concealed`` is then loss only."""
        names, fields = (STATS, _COUNTERS) if self.cn is None else (STATS + CN_STATS, _COUNTERS + _CN_COUNTERS)
        return {k: torch.from_numpy(getattr(self._b, f).copy()) for k, f in zip(names, fields)}

    # ---- planning (host arithmetic only) -----------------------------------------------------------------------------
    def _geometry(self, rate):
        """(L, M, J, W, G, depth, lookback) at the rate indices ``rate``: int64 arrays over them (G: the samples of a gap that
        are not zeros: the fade length F, in "pitch_sync" hold + F)."""
        return tuple(a[rate] for a in (self._rL, self._rM, self._rJ, self._rW, self._rG, self._rdepth, self._rlookback))

    def _unwrap(self, t, ref):
        """Timestamp t as the absolute value nearest ref (ts_bits), or as it is."""
        if self.ts_bits is None:
            return t
        mod = 1 << self.ts_bits
        return ref + ((t - ref + mod // 2) % mod) - mod // 2

    def _place_rows(self, b, slot, size, ts, offs, seqs, encs=None):
        """Phase 1 of a feed: the bookkeeping of every row, in order -> placements (int64 arrays: slot, first index, n, byte
        offset, encoding number).  Rows that continue a hole-free slot at its ``hi`` (the common case) are handled for all
        slots at once; the others one by one.  ``encs``: the encoding number of every row (None: this scorer's first)."""
        if encs is None:
            encs = self._renc[self._rate_of[slot]]
        bps_of = _BPS[encs]
        once = np.bincount(slot, minlength=self.S)[slot] == 1
        ref = b.origin[slot] + b.hi[slot]
        rel = self._unwrap(ts, ref) - b.origin[slot]
        fast = once & (b.started[slot] == 1) & ~b.holey[slot] & (rel == b.hi[slot])
        place = []
        if fast.any():
            s, n, r = slot[fast], size[fast], rel[fast]
            if seqs is not None:
                q, last = seqs[fast], b.max_seq[s]
                behind = (last >= 0) & (((q - last) & 0xFFFF) >= 0x8000)
                b.ooo[s] += behind
                b.max_seq[s] = np.where(behind, last, q)
            b.max_start[s] = np.maximum(b.max_start[s], r)  # (r = hi >= every earlier start: never out of order)
            b.hi[s] += n
            b.received[s] += n
            keep = n > 0
            place.append(np.stack([s[keep], r[keep], n[keep], offs[fast][keep], encs[fast][keep]]))
        slow = []
        rest = np.flatnonzero(~fast)
        if rest.size:  # plain Python ints over the slots these rows name: read once, written back once
            ss = np.unique(slot[rest])
            keys = ("started", "origin", "next", "hi", "max_start", "max_seq", "ooo", "late", "dup", "received")
            started, origin, nxt_, hi_, max_start, max_seq, ooo, late, dup, received = (
                dict(zip(ss.tolist(), getattr(b, f)[ss].tolist())) for f in keys)
            ivs_of = {}
            seq_rest = [None] * rest.size if seqs is None else seqs[rest].tolist()
            for s, n, t, off, q, enc, bps in zip(slot[rest].tolist(), size[rest].tolist(), ts[rest].tolist(), offs[rest].tolist(), seq_rest,
                                               encs[rest].tolist(), bps_of[rest].tolist()):
                first = not started[s]
                if first:
                    started[s], origin[s], r = 1, t, 0
                else:
                    r = self._unwrap(t, origin[s] + hi_[s]) - origin[s]
                if q is not None:
                    last = max_seq[s]
                    if last >= 0 and ((q - last) & 0xFFFF) >= 0x8000:
                        ooo[s] += 1
                    else:
                        max_seq[s] = q
                elif not first and r < max_start[s]:
                    ooo[s] += 1
                max_start[s] = r if first else max(max_start[s], r)
                lo, hi, nxt = r, r + n, nxt_[s]
                if lo < nxt:
                    late[s] += min(hi, nxt) - lo
                    lo = min(hi, nxt)
                if lo >= hi:
                    continue
                ivs = ivs_of[s] if s in ivs_of else b.intervals(s)
                new = _subtract(lo, hi, ivs)
                got = sum(e - a for a, e in new)
                dup[s] += hi - lo - got
                received[s] += got
                for a, e in new:
                    slow.append((s, a, e - a, off + (a - r) * bps, enc))
                hi_[s] = max(hi_[s], hi)
                ivs_of[s] = _merge([list(v) for v in ivs], new)
            order = ss.tolist()
            for f, d in zip(keys, (started, origin, nxt_, hi_, max_start, max_seq, ooo, late, dup, received)):
                getattr(b, f)[ss] = [d[s] for s in order]
            for s, ivs in ivs_of.items():
                b.set_intervals(s, ivs)
        if slow:
            place.append(np.array(slow, dtype=np.int64).T)
        return np.concatenate(place, axis=1) if place else np.zeros((5, 0), dtype=np.int64)

    def _take_gaps(self, b, U, tgt):
        """Phase 2: the named slots U release [next, tgt) -> ({position in U: [[origin, lo, hi], ...]} (the loss gaps of that
        range, in order), {position in U: [[lo, hi, level], ...]} (its comfort-noise parts)), and the bookkeeping moves to
        next = tgt.  Per-slot work only for slots with holes or marks."""
        nxt = b.next[U].copy()
        gaps, noise = {}, {}
        moved = tgt > nxt
        plain = moved & ~b.holey[U]
        b.gap[U[plain]] = -1
        b.next[U[plain]] = tgt[plain]
        if self.cn is not None:
            b.cn_open[U[plain]] = -1
        for u in np.flatnonzero(moved & b.holey[U]).tolist():
            s, lo, hi = int(U[u]), int(nxt[u]), int(tgt[u])
            ivs = b.holes[s]
            g = _subtract(lo, hi, ivs)
            level = -1
            if g:
                opened = int(b.gap[s])
                gl = [[opened if k == 0 and a == lo and opened >= 0 else a, a, e] for k, (a, e) in enumerate(g)]
                origin = gl[-1][0]
                marks, level = b.marks.get(s), int(b.cn_open[s]) if gl[0][0] != gl[0][1] else -1
                if marks or level >= 0:  # split at the governing marks: loss before the first of a run, noise from it on
                    loss, nz = [], []
                    for o, a, e in gl:
                        level = level if o != a else -1  # (a run that began before this release keeps the level in force)
                        for t, l in marks or ():
                            if a <= t < e:
                                if t > a:
                                    loss.append([o, a, t]) if level < 0 else nz.append([a, t, level])
                                a, level = t, l
                        loss.append([o, a, e]) if level < 0 else nz.append([a, e, level])
                    gl = loss
                    noise[u] = nz
                    b.comfort[s] += sum(e - a for a, e, _ in nz)
                if gl:
                    gaps[u] = gl
                b.concealed[s] += sum(e - a for _, a, e in gl)
            open_ = bool(g) and g[-1][1] == hi
            b.gap[s] = origin if open_ else -1
            b.cn_open[s] = level if open_ else -1
            b.next[s] = hi
            b.set_intervals(s, [[max(a, hi), e] for a, e in ivs if e > hi])
        if b.marks:  # marks are dropped as the playout point passes them
            for s, up in zip(U.tolist(), tgt.tolist()):
                if s in b.marks and b.marks[s][0][0] < up:
                    b.marks[s] = [m for m in b.marks[s] if m[0] >= up]
                    if not b.marks[s]:
                        del b.marks[s]
        return gaps, noise

    def _mark_rows(self, b, slot, ts, level):
        """The silence marks (slot[i], timestamp ts[i], level[i]) go into the book ``b``, in order."""
        for s, t, l in zip(slot, ts, level):
            if not b.started[s]:
                b.marks_late[s] += 1
                continue
            origin = int(b.origin[s])
            r = self._unwrap(t, origin + int(b.hi[s])) - origin
            have = b.marks.get(s, [])
            if r < b.next[s]:
                b.marks_late[s] += 1
            elif all(m[0] != r for m in have):  # (of two marks at one t the first arrival wins)
                b.marks[s] = sorted(have + [[r, l]])
                b.nmarks[s] += 1

    def _plan(self, slots, sizes=None, ts=None, offs=None, seqs=None, mode="feed", upto=None, score=True, encs=None, marks=None):
        """The launches of a call over the rows ``slots`` (feed: sizes[i] samples with timestamp ts[i] and payload at byte
        offs[i] for slots[i], a slot possibly named more than once; flush / advance / drain: distinct slots) -> Plan.  No
        state changes here: ``_commit(plan.book)`` (or ``_run``) makes it so.  ``marks``: (slots, timestamps, levels) of
        the silence marks the call brings, registered before its rows are planned."""
        b = self._b.copy()
        if marks is not None:
            self._mark_rows(b, *marks)
        R, hop = self.ring_len, self.hop
        slot = np.asarray(slots, dtype=np.int64).reshape(-1)
        if mode == "feed":
            pl = self._place_rows(b, slot, np.asarray(sizes, dtype=np.int64).reshape(-1), np.asarray(ts, dtype=np.int64).reshape(-1),
                                  np.asarray(offs, dtype=np.int64).reshape(-1), None if seqs is None else np.asarray(seqs, dtype=np.int64),
                                  None if encs is None else np.asarray(encs, dtype=np.int64).reshape(-1))
        else:
            pl = np.zeros((5, 0), dtype=np.int64)
        _, first = np.unique(slot, return_index=True)
        first.sort()
        U = slot[first]  # the named slots, once each, in the order they were first named
        rate = self._rate_of[U]
        L, M, J, W, F, depth, _ = self._geometry(rate)  # (int64 arrays over U, each slot with its own rate's values)
        pitch, Lh = self.conceal == "pitch_sync", (self._rPmax + self._rWc)[rate]
        cur = b.next[U].copy()
        if mode == "feed":
            tgt = np.maximum(cur, b.hi[U] - depth)
        elif mode == "flush":
            tgt = b.hi[U].copy()
        elif mode == "advance":
            tgt = np.maximum(cur, np.broadcast_to(np.asarray(upto, dtype=np.int64), U.shape))
            for u in np.flatnonzero(tgt > b.hi[U]).tolist():  # playout beyond everything received: a gap up to there
                s = int(U[u])
                ivs = b.intervals(s)
                b.hi[s] = tgt[u]
                b.set_intervals(s, [list(v) for v in ivs])
        else:
            tgt = cur.copy()
        if not score:
            after = b.fill[U] - (-tgt * L // M) + (-cur * L // M)
            over = np.flatnonzero(after > self.max_pending * hop)
            if over.size:
                raise ValueError(f"slot {U[over[0]]} would hold {after[over[0]]} pending samples, more than max_pending = "
                                 f"{self.max_pending} hops of {hop}: drain it first")
        gaps, noise = self._take_gaps(b, U, tgt)
        pos = np.full(self.S, -1, dtype=np.int64)
        pos[U] = np.arange(U.size)
        pu, pstart, pn, poff, penc = pos[pl[0]], pl[1], pl[2], pl[3], pl[4]
        bps = _BPS[penc]
        pdone = np.zeros_like(pn)
        head, fill = b.head[U].copy(), b.fill[U].copy()
        counts = np.zeros(U.size, dtype=np.int64)
        ops = []
        while True:
            progress = False
            # place what the window [cur, cur + W) of each slot takes
            take = np.clip(cur[pu] + W[pu] - (pstart + pdone), 0, pn - pdone)
            k = np.flatnonzero(take > 0)
            if k.size:
                cols = [U[pu[k]], poff[k] + pdone[k] * bps[k], take[k], (pstart[k] + pdone[k]) % J[pu[k]]] + (
                    [penc[k]] if self._mixed else []) + ([rate[pu[k]]] if self._rated else [])
                rows = np.stack(cols, axis=1).astype(np.int32)
                ops.append(("place", rows, int(take[k].max())))
                pdone[k] += take[k]
                progress = True
            # release what is due, the window holds and the pending ring has room for
            made = -(-cur * L // M)
            m = np.maximum(np.minimum(np.minimum(tgt - cur, W), (made + R - fill) * M // L - cur), 0)
            rows = []
            for u, nl in noise.items():  # the noise parts inside [cur, cur + m): one launch (noise has no source, so no ranks)
                c0, c1, s, Ju = int(cur[u]), int(cur[u] + m[u]), int(U[u]), int(J[u])
                tail = (int(rate[u]),) if self._rated else ()
                for lo, hi, level in nl:
                    lo, hi = max(lo, c0), min(hi, c1)
                    if lo < hi:
                        rows.append((s, lo % Ju, hi - lo, lo & _M32, lo >> 32, level) + tail)
            if rows:
                rows = np.array(rows, dtype=np.int64)
                ops.append(("noise", rows.astype(np.int32), int(rows[:, 2].max())))  # (lo32 keeps its bits as an int32)
            ranks, opens = [], []  # per rank: the conceal rows, and ("pitch_sync") the rows of the gaps whose origin is released
            for u, gl in gaps.items():  # the gaps inside [cur, cur + m) of the slots that have any, by rank within the slot
                c0, c1, s, rank, Fu, Ju = int(cur[u]), int(cur[u] + m[u]), int(U[u]), 0, int(F[u]), int(J[u])
                tail = (int(rate[u]),) if self._rated else ()
                for a, lo, hi in gl:
                    lo, hi = max(lo, c0), min(hi, c1)
                    if lo >= hi:
                        continue
                    d_lo, d_hi = lo - a, hi - a
                    if d_lo >= Fu:  # all zeros from here on: the same row counted from a + d_lo - F (d stays small)
                        a, d_lo, d_hi = a + d_lo - Fu, Fu, Fu + d_hi - d_lo
                    if rank == len(ranks):
                        ranks.append([])
                        opens.append([])
                    ranks[rank].append((s, a % Ju, d_lo, d_hi) + tail)
                    if pitch and d_lo == 0:  # p* is fixed here, from E as it stands before this rank's conceal
                        opens[rank].append((s, a % Ju) + tail)
                    rank += 1
            for rows, first_rows in zip(ranks, opens):
                if first_rows:
                    ops.append(("pitch", np.array(first_rows, dtype=np.int32), int(Lh[pos[[r[0] for r in first_rows]]].max())))
                rows = np.array(rows, dtype=np.int32)
                ops.append(("conceal", rows, int((rows[:, 3] - rows[:, 2]).max())))
            k = np.flatnonzero(m > 0)
            if k.size:
                Lk, Mk = L[k], M[k]
                n_out = -(-(cur[k] + m[k]) * Lk // Mk) - made[k]
                rows = np.zeros((k.size, RELEASE_HDR), dtype=np.int32)
                for c, v in enumerate((U[k], cur[k] % J[k], m[k], n_out, made[k] * Mk % Lk, made[k] * Mk // Lk - cur[k],
                                       (head[k] + fill[k]) % R, rate[k] if self._rated else 0)):
                    rows[:, c] = v
                ops.append(("release", rows, int(n_out.max())))
                if self._prov is not None:
                    ops.extend(self._span_rows(k, U[k], (head[k] + fill[k]) % R, cur[k], m[k], made[k], n_out, Lk, Mk, gaps, noise))
                cur[k] += m[k]
                fill[k] += n_out
                progress = True
            if score and self._pop_rounds(ops, U, head, fill, counts):
                progress = True
            if (pdone == pn).all() and (cur == tgt).all():
                break
            if not progress:
                raise RuntimeError("the jitter plan made no progress")  # (validated before planning: not reached)
        b.head[U], b.fill[U] = head, fill
        per_row = np.zeros(slot.size, dtype=np.int64)
        per_row[first] = counts  # a slot named twice: its hops are counted at its first row
        return Plan(ops, U.tolist(), per_row, b)

    def _span_rows(self, k, slot, wpos, cur, m, made, n_out, L, M, gaps, noise):
        """The ("spans", rows, longest row) ops of a round's release rows (``k``: their positions in U; the other arrays over
        them; one op, or one per ``SPANS_MAX_ROWS`` rows: a slot's release may be cut into many runs): rows of (slot, wpos, n, value) that partition each release row's outputs [made, made + n_out), written from
        ring position wpos on, into received runs (0) and synthetic runs (1).  A loss or noise part [u, v) of the released
        range is the outputs [ceil(u L / M), ceil(v L / M)) (``afx.provenance``); a release with nothing synthetic is one row
        of zeros."""
        R = self.ring_len
        marked = np.array([u in gaps or u in noise for u in k.tolist()], dtype=bool)
        rows = np.stack([slot, wpos, n_out, np.zeros_like(n_out)], axis=1)[~marked].tolist()
        for j in np.flatnonzero(marked).tolist():
            u, c0, c1, l, mm = int(k[j]), int(cur[j]), int(cur[j] + m[j]), int(L[j]), int(M[j])
            s, w, base, end = int(slot[j]), int(wpos[j]), int(made[j]), int(made[j] + n_out[j])
            parts = [(g[1], g[2]) for g in gaps.get(u, ())] + [(z[0], z[1]) for z in noise.get(u, ())]
            at, first = base, len(rows)
            for lo, hi in sorted((max(lo, c0), min(hi, c1)) for lo, hi in parts):
                if lo >= hi:
                    continue
                o0, o1 = -(-lo * l // mm), -(-hi * l // mm)  # base <= o0 <= o1 <= end
                if o0 > at:
                    rows.append((s, (w + at - base) % R, o0 - at, 0))
                if o1 > o0:
                    rows.append((s, (w + o0 - base) % R, o1 - o0, 1))
                at = o1
            if end > at or len(rows) == first:
                rows.append((s, (w + at - base) % R, end - at, 0))
        rows = np.array(rows, dtype=np.int64).reshape(-1, 4).astype(np.int32)
        return [("spans", part, int(part[:, 2].max())) for part in (rows[i:i + SPANS_MAX_ROWS] for i in range(0, len(rows), SPANS_MAX_ROWS))]

    def _span_launch(self):
        """The launch of a "spans" op, for a scorer whose provenance lane is on."""
        if self._prov is None:
            return {}

        def spans(d, off, op):
            check(call_on(self.psyn, lib().afx_k_prov_spans, ptr(self.psyn), self.S, self.ring_len, _at(d, off), len(op[1]), op[2]))
        return {"spans": spans}

    def _note_pop(self, d, off, op):
        """The popped hops' marks become frame counts (one ``afx_k_prov_frames`` launch over the pop's own table) and are noted
        to the attached gate, or as one count per hop to the provenance layer."""
        if self._prov is None:
            return
        target, frame, gated = self._prov
        counts = torch.empty(len(op[2]), self.hop // frame, dtype=torch.int32, device=self.device)
        check(call_on(self.psyn, lib().afx_k_prov_frames, ptr(self.psyn), self.S, self.ring_len, _at(d, off), len(op[2]), self.hop,
                      frame, ptr(counts)))
        target.note_synthetic(counts if gated else counts.view(-1), op[2])

    def _commit(self, book):
        self._b = book

    # ---- the public calls --------------------------------------------------------------------------------------------
    def _rows(self, slots, repeats=False):
        """``slots`` -> list of slot indices in the order given (a bool mask: ascending); repeats: a slot may be named more
        than once."""
        if not repeats:
            return self.scorer._slot_list(slots, ordered=True)
        t = torch.as_tensor(slots)
        if t.numel() == 0 and t.ndim <= 1:
            return []
        if t.dtype == torch.bool or t.is_floating_point() or t.is_complex() or t.ndim > 1:
            raise ValueError("slots: a list of slot indices (a slot may be named more than once)")
        idx = t.reshape(-1).cpu().numpy()
        bad = idx[(idx < 0) | (idx >= self.S)]
        if bad.size:
            raise ValueError(f"slot index {bad[0]} outside 0..{self.S - 1}")
        return idx.tolist()

    def _timestamps(self, timestamps, n):
        if isinstance(timestamps, torch.Tensor):
            timestamps = timestamps.detach().cpu().numpy()
        try:
            vals = np.asarray(timestamps)
        except (OverflowError, ValueError):
            vals = np.zeros(0, dtype=object)
        if vals.ndim != 1 or (vals.size and vals.dtype.kind not in "iu"):
            raise ValueError("timestamps: a list of ints or a 1-D integer array, in input-rate samples")
        if vals.size != n:
            raise ValueError(f"{vals.size} timestamps for {n} named slots")
        lim = 1 << (self.ts_bits if self.ts_bits is not None else 62)
        low = 0 if self.ts_bits is not None else -lim
        if vals.size and (vals.dtype == np.uint64 and int(vals.max()) >= lim or int(vals.min()) < low or int(vals.max()) >= lim):
            raise ValueError(f"a timestamp outside {low}..{lim - 1}" + (f" (ts_bits = {self.ts_bits})" if self.ts_bits else ""))
        return vals.astype(np.int64)

    def feed(self, packets, slots, timestamps, score=True, _seqs=None, encodings=None, _marks=None):
        """packets[i]: a packet of slot slots[i] whose first sample has timestamp timestamps[i] (Python ints or an int64
        array, in input-rate samples), any length, in any order; a slot may be named more than once (its rows are taken in
        the order given).  Afterwards each named slot has released [next, max(next, hi - depth)).  score=True: every hop a
        named slot completes is scored; score=False: buffered only (``drain`` scores them; a slot whose buffer would hold
        more than ``max_pending`` hops is a ValueError).  Everything is checked before anything changes.  -> FeedResult
        with one count per row of ``slots`` (a slot named twice has its hops at its first row).  ``encodings``: the encoding
        of every packet, each one of this scorer's listed encodings (None: the first listed, for all)."""
        return self._run(*self._plan_feed(packets, slots, timestamps, score, _seqs, encodings, _marks))

    def _plan_feed(self, packets, slots, timestamps, score=True, seqs=None, encodings=None, marks=None):
        """The checks and the plan of a ``feed`` -> (Plan, payload blocks).  No state changes.  ``marks``: as for ``_plan``."""
        idx = self._rows(slots, repeats=True)
        ri = self._rate_of[np.asarray(idx, dtype=np.int64)]
        if encodings is None:  # the first listed at each slot's rate
            encs = self._rdefault[ri]
            names = np.array(_NAMES, dtype=object)[encs].tolist()
        else:
            if isinstance(encodings, str) or not hasattr(encodings, "__len__"):
                raise ValueError("encodings: one encoding per packet")
            names = list(encodings)
            if len(names) != len(idx):
                raise ValueError(f"{len(names)} encodings for {len(idx)} named slots")
            try:  # (a name that is no encoding at all gets the number of the table's last column, where nothing is listed)
                encs = np.fromiter(map(_HOST_NUMBER.get, names, repeat(len(_NAMES))), dtype=np.int64, count=len(names))
            except TypeError:
                raise ValueError("encodings: one encoding per packet") from None
            bad = np.flatnonzero(~self._listed[ri, encs])
            if bad.size:
                i, r = int(bad[0]), int(ri[bad[0]])
                what = f"encoding {names[i]!r} is not one of this scorer's {self._encs_at[r]}"
                raise ValueError(f"slot {idx[i]}: {what} at {self._rates[r]} Hz" if self._rated else what)
        unit = _HOST_UNIT[encs]
        pay, nbytes = self._packets_each(packets, names, unit)
        ts = self._timestamps(timestamps, len(idx))
        offs, total = layout(nbytes)
        # a packet in a codec is, for the planner, a pcm_f32le block of the decoded zone (afx.ingest.expand_zone)
        codec = encs - len(ENCODINGS)
        n, offs, rows, zone = expand_zone(nbytes, offs, total, codec)
        if total + zone >= 1 << 31:
            raise ValueError("a feed carries less than 2 GiB")
        plan = self._plan(idx, np.where(codec >= 0, n, nbytes // unit), ts, offs, seqs, "feed", score=score,
                          encs=np.where(codec >= 0, 0, encs), marks=marks)
        plan.ops = with_expand(plan.ops, rows)
        return plan, pay

    def silence(self, slots, timestamps, levels):
        """Silence marks (module docstring): from timestamps[i] on, slot slots[i] is silent with a background noise
        ``levels[i]`` dB below overload (an int in 0..127).  A slot may be named more than once; timestamps as for ``feed``.
        Host only: nothing is released or launched.  Everything is checked before anything changes; a scorer without a
        ``ComfortNoise`` refuses."""
        if self.cn is None:
            raise ValueError("silence: this scorer has no ComfortNoise (comfort_noise=)")
        idx = self._rows(slots, repeats=True)
        ts = self._timestamps(timestamps, len(idx))
        b = self._b.copy()
        self._mark_rows(b, idx, ts.tolist(), self._levels(levels, len(idx)))
        self._commit(b)

    @staticmethod
    def _levels(levels, n):
        if isinstance(levels, (torch.Tensor, np.ndarray)):
            levels = levels.tolist()
        if isinstance(levels, (str, bytes)) or not hasattr(levels, "__len__") or len(levels) != n:
            raise ValueError(f"levels: one int in 0..127 per named slot ({n})")
        for l in levels:
            if isinstance(l, bool) or not isinstance(l, (int, np.integer)) or not 0 <= l <= 127:
                raise ValueError(f"level {l!r}: an int in 0..127")
        return [int(l) for l in levels]

    def _rtp_types(self, payload_types):
        """What ``feed_rtp`` looks a payload type up in: 0 is mulaw and 8 alaw (RFC 3551), the other static audio types
        (``rtp.STATIC_AUDIO_FORMATS``) whose clock rate is this scorer's, and ``payload_types`` adds to them."""
        cn = {} if self.cn is None else {rtp.CN_PAYLOAD_TYPE: "cn"}
        static = {pt: e for pt, (r, e) in rtp.STATIC_AUDIO_FORMATS.items() if r == self.input_rate}
        return {**static, **rtp.STATIC_PAYLOAD_TYPES, **cn, **(payload_types or {})}

    def _rtp_encoding(self, s, pt, types):
        """The encoding of a datagram of slot s with payload type pt ("cn": a silence mark), or the ValueError."""
        if self.cn is not None and types.get(pt) == "cn":
            return "cn"
        if types.get(pt) not in self.encodings:
            raise ValueError(f"slot {s}: RTP payload type {pt} is not this scorer's {' / '.join(self.encodings)}")
        return types[pt]

    def feed_rtp(self, datagrams, slots, payload_types=None, score=True, ignore_types=()):
        """datagrams[i]: one RTP datagram (RFC 3550) of slot slots[i].  Its payload type must name this scorer's encoding (one
        of its listed encodings): 0 is mulaw and 8 alaw (RFC 3551), ``payload_types`` ({number: encoding}) adds the dynamic
        ones; its SSRC must be the session's (the first datagram after ``reset`` sets it).  Placement uses the timestamps; the sequence numbers only
        count packets out of order for ``stats()``.  Anything else is a ValueError before anything changes.
        With a ``ComfortNoise``, a datagram of type 13 (RFC 3389), or of a type ``payload_types`` maps to "cn", is a
        silence mark at its timestamp with level payload[0] & 0x7f (an empty payload is a ValueError); all marks of a call
        are registered before its audio is planned.  ``ignore_types``: datagrams of these payload types (RFC 4733
        telephone-events, typically 101) are parsed and SSRC-checked, then dropped.  Marks and dropped datagrams count 0
        hops at their rows; a slot's hops are at its first audio row."""
        args, kw, audio, n, ssrc = self._rtp_rows(datagrams, slots, payload_types, ignore_types)
        res = self.feed(*args, score=score, **kw)
        for s, v in ssrc.items():
            self._b.ssrc[s] = v
        if len(audio) != n:  # the hops of the audio rows at their places among all rows
            counts = torch.zeros(n, dtype=torch.int64)
            counts[audio] = res.counts
            res = type(res)(counts, res.scores)
        return res

    def _plan_rtp(self, datagrams, slots, payload_types=None, score=True, ignore_types=()):
        """The checks and the plan of a ``feed_rtp`` -> (Plan, payload blocks, {slot: its session's SSRC}).  No state changes."""
        args, kw, audio, n, ssrc = self._rtp_rows(datagrams, slots, payload_types, ignore_types)
        plan, pay = self._plan_feed(*args, score, kw["_seqs"], kw["encodings"], kw.get("_marks"))
        if len(audio) != n:
            counts = np.zeros(n, dtype=np.int64)
            counts[audio] = plan.counts
            plan.counts = counts
        return plan, pay, ssrc

    def _rtp_rows(self, datagrams, slots, payload_types, ignore_types):
        """The checks of a ``feed_rtp`` -> (the positional and keyword arguments of the ``feed`` of its audio rows, their
        positions among all rows, the number of rows, {slot: its session's SSRC}).  No state changes."""
        idx = self._rows(slots, repeats=True)
        if isinstance(datagrams, (bytes, bytearray, memoryview)):
            raise ValueError("datagrams: a list with one datagram per named slot")
        pk = [rtp.parse(d) for d in datagrams]
        if len(pk) != len(idx):
            raise ValueError(f"{len(pk)} datagrams for {len(idx)} named slots")
        if self.ts_bits != 32:
            raise ValueError("feed_rtp: RTP timestamps are 32 bits wide (ts_bits = 32)")
        types = self._rtp_types(payload_types)
        try:
            ignore = frozenset(ignore_types)
        except TypeError:
            ignore = None
        if ignore is None or any(isinstance(t, bool) or not isinstance(t, (int, np.integer)) or not 0 <= t <= 127 for t in ignore):
            raise ValueError("ignore_types: payload type numbers, 0..127")
        ssrc, encs, audio, marks = {}, [], [], ([], [], [])
        for i, (s, p) in enumerate(zip(idx, pk)):
            enc = None if p.payload_type in ignore else self._rtp_encoding(s, p.payload_type, types)
            mine = ssrc.setdefault(s, int(self._b.ssrc[s]) if self._b.ssrc[s] >= 0 else p.ssrc)
            if p.ssrc != mine:
                raise ValueError(f"slot {s}: SSRC {p.ssrc:#010x} is not the session's {mine:#010x}")
            if enc == "cn":
                if not len(p.payload):
                    raise ValueError(f"slot {s}: a comfort-noise datagram without a payload (RFC 3389: the first byte is the level)")
                for col, v in zip(marks, (s, p.timestamp, p.payload[0] & 0x7F)):
                    col.append(v)
            elif enc is not None:
                audio.append(i)
                encs.append(enc)
        kw = dict(_seqs=[pk[i].seq for i in audio], encodings=encs if self._mixed else None)
        if marks[0]:
            kw["_marks"] = marks
        return ([pk[i].payload for i in audio], [idx[i] for i in audio], [pk[i].timestamp for i in audio]), kw, audio, len(idx), ssrc

    def flush(self, slots=None, score=True):
        """The named (default: all) slots release everything received, up to ``hi`` -> FeedResult."""
        idx = list(range(self.S)) if slots is None else self._rows(slots)
        return self._run(self._plan(idx, mode="flush", score=score), [])

    def advance(self, slots, upto, score=True):
        """The named slots release up to index ``upto`` of their streams (one int, or one per slot; input-rate samples from
        the session's origin): clock-driven playout of a stream that has gone quiet.  A slot already beyond it is left
        alone; beyond ``hi`` the stream is a gap, and ``hi`` moves there -> FeedResult."""
        idx = self._rows(slots)
        up = np.asarray(upto)
        if up.dtype.kind not in "iu" or up.ndim > 1 or (up.ndim == 1 and up.size != len(idx)) or (up.size and (up.min() < 0 or up.max() >= 1 << 62)):
            raise ValueError("advance: upto is one non-negative integer, or one per named slot")
        up = np.broadcast_to(up.astype(np.int64), (len(idx),))
        cold = [s for s, v in zip(idx, up.tolist()) if not self._b.started[s] and v > 0]
        if cold:
            raise ValueError(f"slot {cold[0]} has no session yet: its origin is its first packet's timestamp")
        return self._run(self._plan(idx, mode="advance", upto=up, score=score), [])

    def drain(self, slots=None):
        """Score every completed hop of the named (default: all) slots -> FeedResult.  Nothing is released."""
        idx = list(range(self.S)) if slots is None else self._rows(slots)
        return self._run(self._plan(idx, mode="drain"), [])

    def _run(self, plan, pay):
        enc, (taps, L, M, T) = device_encoding(self.encoding)[0], self._filter()
        l, S, J = lib(), self.S, self.J

        def place(d, off, op):
            if self._mixed:  # (the rows carry their encoding)
                check(call_on(self.jring, l.afx_k_jitter_place_mixed, _at(d, 0), d.numel(), _at(d, off), len(op[1]), op[2],
                              ptr(self.jring), S, J))
                return
            check(call_on(self.jring, l.afx_k_jitter_place, _at(d, 0), d.numel(), _at(d, off), len(op[1]), op[2], enc, ptr(self.jring),
                          S, J))

        def conceal(d, off, op):
            if self.conceal == "pitch_sync":  # (the period of each row is the device's: what the estimate wrote for its gap)
                check(call_on(self.jring, l.afx_k_jitter_conceal_period, ptr(self.jring), S, J, _at(d, off), len(op[1]), op[2],
                              ptr(self.fade), ptr(self.jperiod), *self.lags, self.period, self.hold, self.fade_len))
                return
            check(call_on(self.jring, l.afx_k_jitter_conceal, ptr(self.jring), S, J, _at(d, off), len(op[1]), op[2], ptr(self.fade),
                          self.period, self.fade_len, CONCEAL.index(self.conceal)))

        def pitch(d, off, op):
            check(call_on(self.jring, l.afx_k_jitter_pitch, ptr(self.jring), S, J, _at(d, off), len(op[1]), *self.lags, self.corr,
                          self.period, ptr(self.jperiod)))

        def release(d, off, op):
            check(call_on(self.jring, l.afx_k_jitter_release, ptr(self.jring), S, J, _at(d, off), len(op[1]), op[2], taps, L, M, T,
                          ptr(self.ring), self.ring_len))

        def noise(d, off, op):
            check(call_on(self.jring, l.afx_k_jitter_noise, ptr(self.jring), S, J, _at(d, off), len(op[1]), op[2], self.cn.seed,
                          ptr(self._amp)))

        return self._execute(plan.ops, plan.slots, plan.counts, pay,
                             {"place": place, "noise": noise, "pitch": pitch, "conceal": conceal, "release": release, **self._span_launch()},
                             lambda: self._commit(plan.book))

    # ---- sessions ----------------------------------------------------------------------------------------------------
    def reset(self, slots):
        """The named slots begin a new stream: inner session, reorder ring, pending samples, origin and counters are dropped."""
        idx = self.scorer._slot_list(slots)
        self.scorer.reset(idx)
        if idx:
            self._b.clear(idx)
            self.jring[idx] = 0.0
            if self.conceal == "pitch_sync":
                self.jperiod[idx] = 0

    def _meta(self):
        return dict(input_rate=self.input_rate, resampler=FILTER_ID, jitter=JITTER_FORMAT, jitter_depth=self.depth,
                    jitter_conceal=self.conceal, jitter_period=self.period, jitter_fade=self.fade_len, **self._cn_meta(),
                    **self._pitch_meta(0))

    def _pitch_meta(self, r):
        """What a state says of the "pitch_sync" function at rate index r beyond period and fade (other modes: nothing)."""
        if self.conceal != "pitch_sync":
            return {}
        return dict(jitter_hold=int(self._rHd[r]), jitter_lags=(int(self._rPmin[r]), int(self._rPmax[r]), int(self._rWc[r])))

    def _pitch_keys(self):
        return ("jitter_pitch",) if self.conceal == "pitch_sync" else ()

    def _cn_meta(self):
        return {} if self.cn is None else dict(jitter_cn=self.cn.seed)

    def _syn_keys(self, state):
        """What ``peel`` takes of ``state``'s provenance marks.  A state with them is refused by a chain without the layer; a
        state without them imports with zeros."""
        has = isinstance(state, StreamState) and "jitter_syn" in state.tensors
        if has and self._prov is None:
            raise ValueError("import_slots: the state carries provenance marks (jitter_syn) and this chain has no provenance layer")
        return ("jitter_syn",) if has else ()

    def _cn_part(self, state, mine):
        """What ``peel`` takes of ``state``'s comfort-noise part -> (its state keys, ``mine`` as far as the state must match
        it).  A state with marks is refused by a scorer without a ``ComfortNoise``; a state without them imports with none."""
        has = isinstance(state, StreamState) and "jitter_cn" in state.meta
        if has and self.cn is None:
            raise ValueError(f"import_slots: the state carries comfort noise (jitter_cn {state.meta['jitter_cn']!r}) and this scorer "
                             "has no ComfortNoise")
        return (_CN_KEYS, mine) if has else ((), {k: v for k, v in mine.items() if k != "jitter_cn"})

    def export_slots(self, slots):
        """The inner scorer's ``StreamState`` of the named slots plus their jitter-buffer sessions (module docstring).  What is
        stored is decoded.  No byte of the scorer changes."""
        return self._export(self.scorer._slot_list(slots, ordered=True))

    def _export(self, idx, **more):
        """``export_slots`` of the slots ``idx``; ``more``: tensors a subclass adds.  ``jitter_ring`` is as wide as the widest
        lookback + depth of this scorer's rates, zeros beyond what a session holds."""
        st = self.scorer.export_slots(idx)
        dev, b = self.device, self._b
        _, _, J, _, _, _, lb = (torch.from_numpy(a) for a in self._geometry(self._rate_of[idx]))
        width = int((self._rlookback + self._rdepth).max())
        with _on(dev):
            nxt, held = torch.from_numpy(b.next[idx]), torch.from_numpy(b.hi[idx] - b.next[idx])
            k = torch.arange(width)
            jr = self.jring[rows_on(idx, dev)[:, None], ((nxt[:, None] - lb[:, None] + k) % J[:, None]).to(dev)]
            jr.masked_fill_((k[None, :] >= (lb + held)[:, None]).to(dev), 0.0)
            if self.conceal == "pitch_sync":  # the period of each open loss gap, masked on the device: nothing is read back
                live = torch.from_numpy((b.gap[idx] >= 0) & (b.cn_open[idx] < 0)).to(dev)
                more = dict(more, jitter_pitch=(self.jperiod[rows_on(idx, dev)] * live).to(torch.int64))
        ivs = [b.intervals(s) for s in idx]
        K = max([len(v) for v in ivs] + [1])
        table = np.full((len(idx), K, 2), -1, dtype=np.int64)
        for i, v in enumerate(ivs):
            if v:
                table[i, :len(v)] = v
        book = np.stack([getattr(b, f)[idx] for f in _BOOK], axis=1).reshape(len(idx), len(_BOOK))
        stats = np.stack([getattr(b, f)[idx] for f in _COUNTERS], axis=1).reshape(len(idx), len(_COUNTERS))
        if self.cn is not None:
            marks = [b.marks.get(s, []) for s in idx]
            mt = np.full((len(idx), max([len(v) for v in marks] + [1]), 2), -1, dtype=np.int64)
            for i, v in enumerate(marks):
                if v:
                    mt[i, :len(v)] = v
            cstats = np.stack([getattr(b, f)[idx] for f in _CN_COUNTERS], axis=1).reshape(len(idx), len(_CN_COUNTERS))
            more = dict(more, jitter_cn_marks=torch.from_numpy(mt), jitter_cn_open=torch.from_numpy(b.cn_open[idx]),
                        jitter_cn_stats=torch.from_numpy(cstats))
        if self._prov is not None:
            more = dict(more, jitter_syn=export_pending(self.psyn, idx, b.head[idx], b.fill[idx], self.max_pending * self.hop))
        return wrap(st, self._meta(), jitter_pending=export_pending(self.ring, idx, b.head[idx], b.fill[idx], self.max_pending * self.hop),
                    jitter_fill=torch.from_numpy(b.fill[idx]), jitter_ring=jr, jitter_book=torch.from_numpy(book),
                    jitter_stats=torch.from_numpy(stats), jitter_intervals=torch.from_numpy(table), **more)

    def import_slots(self, slots, state):
        """The named slots take over the sessions of ``state``, a state of a JitterScorer with the same input rate, filter,
        depth, concealment mode, period and fade whose pending samples fit this scorer's ``max_pending``; anything else,
        or a state whose counters contradict each other, is a ValueError before anything changes.  Comfort noise: a state
        with silence marks needs a ``ComfortNoise`` of its seed here; one without them imports with no marks."""
        idx = self.scorer._slot_list(slots, ordered=True)
        keys, mine = self._cn_part(state, self._meta())
        inner = peel(state, _STATE_KEYS + keys + self._pitch_keys() + self._syn_keys(state), mine,
                     "jitter-buffer part (it was not exported by a JitterScorer)")
        n = len(state)
        width = self.lookback + self.depth
        jr = state.tensors["jitter_ring"]
        if tuple(jr.shape) != (n, width) or jr.dtype != torch.float32:
            raise ValueError(f"import_slots: jitter_ring {tuple(jr.shape)} {jr.dtype} does not fit this scorer ({(n, width)} float32)")
        self._install(idx, inner, self._check_sessions(state, n, np.zeros(n, dtype=np.int64)))

    def _check_sessions(self, state, n, rate):
        """The checks of the jitter part of ``state`` (n sessions, session i at this scorer's rate index rate[i]) -> what
        ``_install`` takes.  A ValueError for counters that contradict each other; nothing changes."""
        L, M, J, _, _, depth, _ = self._geometry(rate)
        pend = state.tensors["jitter_pending"]
        ints = [state.tensors[k].cpu() for k in ("jitter_fill", "jitter_book", "jitter_stats", "jitter_intervals")]
        if any(t.dtype != torch.int64 for t in ints):
            raise ValueError("import_slots: jitter_fill, jitter_book, jitter_stats and jitter_intervals are int64")
        fill, book, stats, table = (t.numpy() for t in ints)
        fill = fill.reshape(-1)
        if fill.size != n or book.shape != (n, len(_BOOK)) or stats.shape != (n, len(_COUNTERS)) or table.ndim != 3 or table.shape[2] != 2:
            raise ValueError("import_slots: jitter_fill (n,), jitter_book (n, 8), jitter_stats (n, 5), jitter_intervals (n, K, 2)")
        check_pending("jitter_pending", pend, fill, n, self.max_pending * self.hop)
        col = {f: book[:, c] for c, f in enumerate(_BOOK)}
        nxt, hi, gap = col["next"], col["hi"], col["gap"]
        made = np.array([-(-int(v) * l // m) for v, l, m in zip(nxt.tolist(), L.tolist(), M.tolist())], dtype=np.int64)
        bad = ((nxt < 0) | (hi < nxt) | (hi - nxt > depth) | ((col["started"] != 0) & (col["started"] != 1)) |
               ((col["started"] == 0) & (hi != 0)) | (gap < -1) | (gap >= nxt) | (stats < 0).any(axis=1) |
               (stats[:, 3] > nxt) | (col["max_seq"] < -1) | (col["max_seq"] > 0xFFFF) | (col["ssrc"] < -1) | (col["ssrc"] >= 1 << 32))
        if bad.any() or not np.array_equal(made, state.seen.numpy() + fill):
            raise ValueError("import_slots: a session's counters contradict each other")
        lists = []
        for i in range(n):
            v = [r for r in table[i].tolist() if r != [-1, -1]]
            ok = all(a < e for a, e in v) and all(p[1] < q[0] for p, q in zip(v, v[1:])) and (not v or (v[0][0] >= nxt[i] and v[-1][1] == hi[i]))
            if not ok or (not v and hi[i] != nxt[i]) or sum(e - a for a, e in v) > stats[i, 0]:
                raise ValueError("import_slots: a session's received intervals contradict its counters")
            lists.append(v)
        cn = None
        if "jitter_cn" in state.meta:
            ints = [state.tensors[k].cpu() for k in _CN_KEYS]
            if any(t.dtype != torch.int64 for t in ints):
                raise ValueError("import_slots: jitter_cn_marks, jitter_cn_open and jitter_cn_stats are int64")
            mt, opened, cstats = (t.numpy() for t in ints)
            opened = opened.reshape(-1)
            if mt.ndim != 3 or mt.shape[0] != n or mt.shape[2] != 2 or opened.size != n or cstats.shape != (n, len(_CN_COUNTERS)):
                raise ValueError("import_slots: jitter_cn_marks (n, K, 2), jitter_cn_open (n,), jitter_cn_stats (n, 3)")
            if ((opened < -1) | (opened > 127) | ((opened >= 0) & (gap < 0)) | (cstats < 0).any(axis=1) |
                    (cstats[:, 0] + stats[:, 3] > nxt)).any():
                raise ValueError("import_slots: a session's comfort-noise counters contradict each other")
            marks = []
            for i in range(n):
                v = [r for r in mt[i].tolist() if r != [-1, -1]]
                if not all(t >= nxt[i] and 0 <= l <= 127 for t, l in v) or not all(p[0] < q[0] for p, q in zip(v, v[1:])) or \
                        len(v) > cstats[i, 1]:
                    raise ValueError("import_slots: a session's silence marks contradict its counters")
                marks.append(v)
            cn = (marks, opened, cstats)
        pit = None
        if self.conceal == "pitch_sync":  # a gap that still sounds needs the period it opened with
            pit = state.tensors["jitter_pitch"].cpu().reshape(-1)
            if pit.dtype != torch.int64 or pit.numel() != n:
                raise ValueError("import_slots: jitter_pitch is (n,) int64")
            pit = pit.numpy()
            sounds = (gap >= 0) & (nxt - gap < self._rG[rate]) & (True if cn is None else cn[1] < 0)
            if ((pit < 0) | (pit > self._rPmax[rate]) | (sounds & (pit < self._rPmin[rate]))).any():
                raise ValueError("import_slots: jitter_pitch holds a period outside its rate's lags for a gap younger than hold + fade")
        syn = state.tensors.get("jitter_syn")
        if syn is not None:  # the marks of the pending samples: laid out as jitter_pending, 0 / 1, zeros after the fill
            if syn.dtype != torch.uint8 or tuple(syn.shape) != tuple(pend.shape):
                raise ValueError(f"import_slots: jitter_syn {tuple(syn.shape)} {syn.dtype} is not {tuple(pend.shape)} uint8, as jitter_pending")
            host = syn.cpu()
            if bool((host > 1).any()) or bool((host * (torch.arange(host.shape[1])[None, :] >= torch.from_numpy(fill)[:, None])).any()):
                raise ValueError("import_slots: jitter_syn marks a sample more than once, or beyond a session's pending samples")
        return pend, state.tensors["jitter_ring"], fill, col, stats, lists, rate, cn, pit, syn

    def _install(self, idx, inner, checked):
        """The inner scorer imports ``inner`` (it refuses a foreign state before changing anything), then the named slots take
        the checked jitter part: ring columns [next - lookback, ...) at their places modulo each session's own J."""
        pend, jr, fill, col, stats, lists, rate, cn, pit, syn = checked
        self.scorer.import_slots(idx, inner)
        if not idx:
            return
        dev, b = self.device, self._b
        if pit is not None:
            self.jperiod[rows_on(idx, dev)] = torch.from_numpy(pit.astype(np.int32)).to(dev)
        _, _, J, _, _, depth, lookback = self._geometry(rate)
        own = lookback + depth  # each session's own columns of jitter_ring
        import_pending(self.ring, idx, pend)
        if self._prov is not None:
            with _on(dev):
                self.psyn[rows_on(idx, dev)] = 0
            if syn is not None:
                import_pending(self.psyn, idx, syn)
        with _on(dev):
            rows = rows_on(idx, dev)
            self.jring[rows] = 0.0
            for w in np.unique(own).tolist():  # (sessions of one rate at a time: a ring row may be wider than their own columns)
                sel = np.flatnonzero(own == w)
                k = torch.arange(w)
                cols = (torch.from_numpy(col["next"][sel].copy())[:, None] - torch.from_numpy(lookback[sel])[:, None] + k) % \
                    torch.from_numpy(J[sel])[:, None]
                self.jring[rows[torch.from_numpy(sel).to(dev)][:, None], cols.to(dev)] = jr[torch.from_numpy(sel)][:, :w].to(dev)
        b.clear(idx)
        for f in _BOOK:
            getattr(b, f)[idx] = col[f]
        for c, f in enumerate(_COUNTERS):
            getattr(b, f)[idx] = stats[:, c]
        b.fill[idx] = fill
        for s_, v in zip(idx, lists):
            b.set_intervals(s_, v)
        if cn is not None:
            marks, b.cn_open[idx], cstats = cn
            for c, f in enumerate(_CN_COUNTERS):
                getattr(b, f)[idx] = cstats[:, c]
            for s_, v in zip(idx, marks):
                if v:
                    b.marks[s_] = v


def _fade_table(F, device):
    return torch.from_numpy((1.0 - np.arange(max(F, 1), dtype=np.float64) / max(F, 1)).astype(np.float32)).to(device)


class MixedJitterScorer(JitterScorer):
    """``scorer`` fed timestamped packets, every slot at its own clock rate: ``formats`` is 1 to 16 distinct
    (input_rate, encoding) pairs; their distinct rates are the scorer's rates, and the encodings listed at a rate are the ones
    a packet of a slot at that rate may come in (the first listed: the default).  ``depth_ms``, ``period_ms`` (default 10)
    and ``fade_ms`` (default three periods) are whole milliseconds; at rate r, depth = depth_ms * r // 1000,
    P = r // 100 (``period_ms`` given: max(1, period_ms * r // 1000)) and F = 3 P (``fade_ms`` given: fade_ms * r // 1000) of
    that rate's samples.  A slot's rate is chosen at ``reset`` (a fresh scorer has every slot at the first format's rate)
    and never changes between resets; everything a ``JitterScorer`` counts in input samples is, per slot, in the slot's own
    rate.  ``feed_rtp`` takes ``payload_types`` as {number: (input_rate, encoding)}.  See the module docstring for the
    contract.  ``comfort_noise``: as for ``JitterScorer``; a CN payload type maps to (input_rate, "cn"), in the slot's clock
    (13 is (8000, "cn"), RFC 3551).  conceal="pitch_sync": P0 = r // 100 (``period_ms`` given: period_ms * r // 1000, inside the
    rate's lags), F = r // 20 (``fade_ms``), Hd = r // 100 (``hold_ms``: hold_ms * r // 1000; this mode only)."""

    _rated = True

    def __init__(self, scorer, formats, depth_ms, conceal="repeat", period_ms=None, fade_ms=None, max_pending=4, ts_bits=32,
                 comfort_noise=None, hold_ms=None):
        if isinstance(formats, (str, bytes)) or not hasattr(formats, "__len__") or not hasattr(formats, "__iter__"):
            raise ValueError("formats: a sequence of (input_rate, encoding) pairs")
        fm = tuple(_format(f) for f in formats)
        if not 1 <= len(fm) <= MAX_FORMATS:
            raise ValueError(f"{len(fm)} formats: 1 to {MAX_FORMATS}")
        if len(set(fm)) != len(fm):
            raise ValueError("formats: a format is listed twice")
        depth_ms = _nonneg_int(depth_ms, "depth_ms")
        period_ms = None if period_ms is None else _nonneg_int(period_ms, "period_ms")
        fade_ms = None if fade_ms is None else _nonneg_int(fade_ms, "fade_ms")
        hold_ms = None if hold_ms is None else _nonneg_int(hold_ms, "hold_ms")
        max_pending = self._checked(conceal, max_pending, ts_bits, comfort_noise)
        if hold_ms is not None and conceal != "pitch_sync":
            raise ValueError(f'hold_ms: a part of conceal="pitch_sync", not of {conceal!r}')
        self.scorer, self.formats, self._mixed = scorer, fm, True
        self.depth_ms, self.period_ms, self.fade_ms, self.hold_ms = depth_ms, period_ms, fade_ms, hold_ms
        rates = tuple(dict.fromkeys(r for r, _ in fm))  # the distinct rates, in the order first listed
        rate = np.array(rates, dtype=np.int64)
        P = F = Hd = np.zeros_like(rate)  # (no part of the "zero" function)
        if conceal == "repeat":
            P = rate // 100 if period_ms is None else np.maximum(1, period_ms * rate // 1000)
            F = 3 * P if fade_ms is None else fade_ms * rate // 1000
        elif conceal == "pitch_sync":
            P = rate // 100 if period_ms is None else period_ms * rate // 1000
            F = rate // 20 if fade_ms is None else fade_ms * rate // 1000
            Hd = rate // 100 if hold_ms is None else hold_ms * rate // 1000
            for r, p in zip(rates, P.tolist()):
                if not pitch_lags(r)[0] <= p <= pitch_lags(r)[1]:
                    raise ValueError(f"period_ms {period_ms}: {p} samples at {r} Hz, outside the lags of the pitch search, "
                                     f"{pitch_lags(r)[0]}..{pitch_lags(r)[1]}")
        self._size([Resampler(r, scorer.device) for r in rates], [tuple(e for q, e in fm if q == r) for r in rates],
                   depth_ms * rate // 1000, P, F, max_pending, Hd)

    # ---- per-slot quantities ---------------------------------------------------------------------------------------------
    @property
    def rates(self):
        """(S,) int64: each slot's clock rate in Hz."""
        return torch.from_numpy(self._rrate[self._rate_of])

    @property
    def depths(self):
        """(S,) int64: each slot's playout delay in its own rate's samples."""
        return torch.from_numpy(self._rdepth[self._rate_of])

    @property
    def periods(self):
        """(S,) int64: each slot's repeat period P in its own rate's samples (0 with conceal="zero")."""
        return torch.from_numpy(self._rP[self._rate_of])

    @property
    def fades(self):
        """(S,) int64: each slot's fade length F in its own rate's samples (0 with conceal="zero")."""
        return torch.from_numpy(self._rF[self._rate_of])

    @property
    def holds(self):
        """(S,) int64: each slot's hold Hd in its own rate's samples (0 outside conceal="pitch_sync")."""
        return torch.from_numpy(self._rHd[self._rate_of])

    @property
    def delays(self):
        """(S,) float64: each slot's ``Resampler.delay``, the lag of its resampled stream in 16 kHz samples."""
        return torch.from_numpy(self._rdelay[self._rate_of])

    @property
    def delay(self):
        raise AttributeError("a MixedJitterScorer has one delay per slot: delays")

    @property
    def depth(self):
        raise AttributeError("a MixedJitterScorer has one depth per slot: depths")

    @property
    def period(self):
        raise AttributeError("a MixedJitterScorer has one period per slot: periods")

    @property
    def input_rate(self):
        raise AttributeError("a MixedJitterScorer has one input rate per slot: rates")

    def _rate_indices(self, rates, n):
        """``rates``: one rate in Hz for n slots, or n of them -> (n,) int64 array of indices into this scorer's rates."""
        if isinstance(rates, (torch.Tensor, np.ndarray)):
            rates = rates.tolist()
        one = isinstance(rates, (int, np.integer)) and not isinstance(rates, bool)
        if not one and (isinstance(rates, (str, bytes)) or not hasattr(rates, "__len__")):
            raise ValueError("rates: one rate in Hz, or one per named slot")
        vals = [rates] * n if one else list(rates)
        if len(vals) != n:
            raise ValueError(f"{len(vals)} rates for {n} named slots")
        for r in vals:
            if isinstance(r, bool) or not isinstance(r, (int, np.integer)) or int(r) not in self._rates:
                raise ValueError(f"rate {r!r} is not one of this scorer's {self._rates}")
        return np.array([self._rates.index(int(r)) for r in vals], dtype=np.int64).reshape(n)

    # ---- the public calls ------------------------------------------------------------------------------------------------
    def _rtp_types(self, payload_types):
        """``feed_rtp`` here takes ``payload_types`` mapping a number to an (input_rate, encoding) pair: 0 and 8 are
        (8000, "mulaw") and (8000, "alaw") (RFC 3551).  A datagram whose type maps to another rate than its slot's, or to a
        pair this scorer does not list, is a ValueError before anything changes."""
        types = {**rtp.STATIC_AUDIO_FORMATS, **{pt: (8000, e) for pt, e in rtp.STATIC_PAYLOAD_TYPES.items()}}
        if self.cn is not None:
            types[rtp.CN_PAYLOAD_TYPE] = (8000, "cn")
        cn = lambda f: self.cn is not None and isinstance(f, (tuple, list)) and len(f) == 2 and f[1] == "cn" and f[0] in self._rates
        types.update((pt, (int(f[0]), "cn") if cn(f) else _format(f)) for pt, f in (payload_types or {}).items())
        return types

    def _rtp_encoding(self, s, pt, types):
        f, mine = types.get(pt), self._rates[self._rate_of[s]]
        cn = self.cn is not None and f is not None and f[1] == "cn"  # a silence mark, in the slot's clock
        if cn and f[0] == mine:
            return "cn"
        if not cn and f not in self.formats:
            raise ValueError(f"slot {s}: RTP payload type {pt} maps to none of this scorer's formats {self.formats}")
        if f[0] != mine:
            raise ValueError(f"slot {s}: RTP payload type {pt} is {f[0]} Hz, the slot is at {mine} Hz")
        return f[1]

    def _run(self, plan, pay):
        l, S, Js, nr = lib(), self.S, self.Js, len(self._rates)
        pitched = self.conceal == "pitch_sync"
        table, mode = C.cast(self._table, C.c_void_p), CONCEAL.index(self.conceal)
        lags = C.cast(self._lags, C.c_void_p) if pitched else None

        def place(d, off, op):
            check(call_on(self.jring, l.afx_k_jitter_place_rates, _at(d, 0), d.numel(), _at(d, off), len(op[1]), op[2], table, nr,
                          ptr(self.jring), S, Js))

        def conceal(d, off, op):
            if pitched:
                check(call_on(self.jring, l.afx_k_jitter_conceal_period_rates, ptr(self.jring), S, Js, _at(d, off), len(op[1]), op[2],
                              table, lags, nr, ptr(self.jperiod)))
                return
            check(call_on(self.jring, l.afx_k_jitter_conceal_rates, ptr(self.jring), S, Js, _at(d, off), len(op[1]), op[2], table, nr,
                          mode))

        def pitch(d, off, op):
            check(call_on(self.jring, l.afx_k_jitter_pitch_rates, ptr(self.jring), S, Js, _at(d, off), len(op[1]), table, lags, nr,
                          ptr(self.jperiod)))

        def release(d, off, op):
            rows = op[1]
            most = np.zeros(nr, dtype=np.int32)  # per rate the largest n_out of this launch
            np.maximum.at(most, rows[:, 7], rows[:, 3])
            check(call_on(self.jring, l.afx_k_jitter_release_rates, ptr(self.jring), S, Js, _at(d, off), len(rows), table, nr,
                          most.ctypes.data_as(C.c_void_p), ptr(self.ring), self.ring_len))

        def noise(d, off, op):
            check(call_on(self.jring, l.afx_k_jitter_noise_rates, ptr(self.jring), S, Js, _at(d, off), len(op[1]), op[2], table, nr,
                          self.cn.seed, ptr(self._amp)))

        return self._execute(plan.ops, plan.slots, plan.counts, pay,
                             {"place": place, "noise": noise, "pitch": pitch, "conceal": conceal, "release": release, **self._span_launch()},
                             lambda: self._commit(plan.book))

    # ---- sessions --------------------------------------------------------------------------------------------------------
    def reset(self, slots, rates=None):
        """The named slots begin a new stream at ``rates``: one rate in Hz for all of them, or one per named slot; None keeps
        each slot's rate.  A rate this scorer does not list is a ValueError before anything changes."""
        idx = self.scorer._slot_list(slots, ordered=True)
        new = None if rates is None else self._rate_indices(rates, len(idx))
        super().reset(idx)
        if idx and new is not None:
            self._rate_of[idx] = new

    def _meta(self):
        return dict(resampler=FILTER_ID, jitter=JITTER_FORMAT, jitter_conceal=self.conceal, jitter_mixed=1, **self._cn_meta())

    def _params(self, ri):
        """``jitter_params`` of sessions at the rate indices ``ri``: depth, period, fade ("pitch_sync": and hold), int64."""
        cols = [self._rdepth[ri], self._rP[ri], self._rF[ri]] + ([self._rHd[ri]] if self.conceal == "pitch_sync" else [])
        return np.stack(cols, axis=1).reshape(len(ri), len(cols))

    def export_slots(self, slots):
        """``JitterScorer.export_slots`` with the per-session ``jitter_rate`` ((n,) int64, Hz) and ``jitter_params`` ((n, 3)
        int64: depth, period, fade in the session's own rate; "pitch_sync": (n, 4), the fourth the hold -- the lags and the
        correlation window are functions of the rate).  No byte of the scorer changes."""
        idx = self.scorer._slot_list(slots, ordered=True)
        ri = self._rate_of[idx]
        params = self._params(ri)
        return self._export(idx, jitter_rate=torch.from_numpy(self._rrate[ri]), jitter_params=torch.from_numpy(params))

    def import_slots(self, slots, state):
        """The named slots take over the sessions of ``state``, each at its own rate: a state of a MixedJitterScorer, or of a
        plain ``JitterScorer`` (one ``input_rate`` in its meta) whose rate is listed here and whose depth, period, fade and
        concealment mode are that rate's here.  A rate this scorer does not list, parameters that differ, ring columns that
        are non-zero beyond a session's own, or anything ``JitterScorer.import_slots`` refuses is a ValueError before
        anything changes."""
        idx = self.scorer._slot_list(slots, ordered=True)
        what = "jitter-buffer part (it was not exported by a JitterScorer or a MixedJitterScorer)"
        n = len(state) if hasattr(state, "seen") else 0
        if hasattr(state, "meta") and "jitter_mixed" not in state.meta and "input_rate" in state.meta:  # a plain JitterScorer's
            rate = state.meta["input_rate"]
            if rate not in self._rates:
                raise ValueError(f"import_slots: a session at {rate} Hz, which is none of this scorer's rates {self._rates}")
            r = self._rates.index(rate)
            mine = dict(input_rate=rate, resampler=FILTER_ID, jitter=JITTER_FORMAT, jitter_depth=int(self._rdepth[r]),
                        jitter_conceal=self.conceal, jitter_period=int(self._rP[r]), jitter_fade=int(self._rF[r]), **self._cn_meta(),
                        **self._pitch_meta(r))
            keys, mine = self._cn_part(state, mine)
            inner = peel(state, _STATE_KEYS + keys + self._pitch_keys() + self._syn_keys(state), mine, what)
            ri = np.full(n, r, dtype=np.int64)
        else:
            keys, mine = self._cn_part(state, self._meta())
            inner = peel(state, _STATE_KEYS + ("jitter_rate", "jitter_params") + keys + self._pitch_keys() + self._syn_keys(state), mine, what)
            rates, params = state.tensors["jitter_rate"].cpu().reshape(-1), state.tensors["jitter_params"].cpu()
            width = 4 if self.conceal == "pitch_sync" else 3
            if rates.dtype != torch.int64 or rates.numel() != n or params.dtype != torch.int64 or tuple(params.shape) != (n, width):
                raise ValueError(f"import_slots: jitter_rate is (n,) int64, jitter_params (n, {width}) int64")
            missing = [r for r in rates.tolist() if r not in self._rates]
            if missing:
                raise ValueError(f"import_slots: a session at {missing[0]} Hz, which is none of this scorer's rates {self._rates}")
            ri = np.array([self._rates.index(r) for r in rates.tolist()], dtype=np.int64)
            here = self._params(ri)
            bad = np.flatnonzero((params.numpy() != here).any(axis=1))
            if bad.size:
                names = "depth, period, fade" + ", hold" * (width == 4)
                raise ValueError(f"import_slots: session {bad[0]} has {names} {params[bad[0]].tolist()}, this scorer's at "
                                 f"{rates[bad[0]]} Hz are {here[bad[0]].tolist()}")
        if len(idx) != n:
            raise ValueError(f"the state holds {n} sessions for {len(idx)} named slots")
        jr = state.tensors["jitter_ring"]
        own = self._rlookback[ri] + self._rdepth[ri]
        if jr.ndim != 2 or jr.shape[0] != n or jr.dtype != torch.float32 or (n and jr.shape[1] < own.max()):
            raise ValueError(f"import_slots: jitter_ring {tuple(jr.shape)} {jr.dtype} does not hold its sessions' columns "
                             f"((n, >= {int(own.max()) if n else 0}) float32)")
        if n and jr.shape[1] and bool((jr.cpu() * (torch.arange(jr.shape[1])[None, :] >= torch.from_numpy(own)[:, None])).ne(0).any()):
            raise ValueError("import_slots: jitter_ring has non-zero columns beyond a session's own lookback + depth")
        self._install(idx, inner, self._check_sessions(state, n, ri))
        if idx:
            self._rate_of[idx] = ri
