"""Speech gate of the streaming scorers: score only the frames with speech.

In a call each direction is silent more than half of the time, a sender's DTX is a gap the jitter buffer fills with zeros,
and the score of a window of line noise says nothing about a speaker.  ``GatedScorer`` stands between the fronts
(``ResamplingScorer``, ``afx.ingest.PacketScorer``, ``afx.jitter.JitterScorer``) and one of the three streaming scorers:
on the GPU ``afx_k_gate`` decides frame by frame which audio is speech, compacts the kept frames into a per-slot ring, and a
slot's inner session advances only when a whole hop of kept audio has accumulated (the inner scorers' non-paced
``push(chunk, slots)``: a tick costs what its active slots cost).

The function (also stated in include/afx.h, afx_k_gate).  The gate works on 16 kHz fp32 samples in frames of ``frame``
samples (160 = 10 ms, the stride of conv layer 5; a scorer's hop must be a multiple of it).  Parameters: ``floor`` (mean
square per sample, default 1e-6 = -60 dBFS), ``ratio`` (8.0), ``rise`` (1.01 per frame), ``hang`` (20 frames) and ``frame``.
Three fp32 constants are derived, each computed in float64 and rounded once: ``E_floor = floor * frame``, ``ratio``,
``rise``; then ``nf_min = fp32(E_floor / ratio)``.  Per stream the state is ``nf`` (fp32, +inf for a new stream) and ``h``
(int, 0 for a new stream).

The energy ``e`` of a frame is the sum of its squared samples in one fixed order, every operation a single correctly
rounded fp32 multiply or add (no fma):

1. ``sq[i] = x[i] * x[i]``;
2. 64 partials ``p[l] = sq[l]``, then ``+ sq[l + 64]``, then ``+ sq[l + 128]``, ... in ascending ``l + 64 k``; indices at or
   beyond ``frame`` contribute nothing (for 160: lanes 0-31 have three terms, lanes 32-63 two);
3. for ``w`` = 32, 16, 8, 4, 2, 1: ``p[l] = p[l] + p[l + w]`` for ``l < w``; ``e = p[0]``

-- a wave-64 strided accumulation and a shuffle-down tree on the device, and exactly what numpy float32 computes in
``frame_energies``.  Per frame, in stream order::

    speech = (e < inf) and e > max(E_floor, ratio * nf)      # fp32 multiply; nf = inf gives inf: not speech
    if e < inf:  nf = max(nf_min, min(e, nf * rise))         # the first frame sets the floor; a non-finite e leaves nf alone
    if speech:   h = hang
    keep = speech or h > 0
    if not speech and h > 0:  h -= 1

The gated stream G of a stream R is the concatenation of R's kept frames, samples copied bit for bit.  Exactly ``hang``
frames after the last speech frame are kept.  There is NO pre-roll: the frames before an onset are not kept.  A stream that
begins in the middle of speech has set its floor from speech and is kept only from its first energy dip of ``ratio`` on
(the floor follows the dip down at once and climbs back by ``rise`` per frame).  The defaults are engineering defaults,
not tuned on data: there is no speech corpus in this repository.

Onset pre-roll by look-ahead (``LookaheadGate``; also stated in include/afx.h, afx_k_gate_la).  The plain gate hands the
model every talk spurt with its first consonant cut at a frame edge.  ``LookaheadGate(floor, ratio, rise, hang, frame, pre)``
has one more parameter, ``pre``: frames of pre-roll, 1 <= pre <= 31, default 5 = 50 ms (an engineering default too).  The
decision per frame above is unchanged -- the energy order, ``speech``, the ``nf`` update, ``h`` and ``keep``.  On top of it
sits a delay line of ``pre`` frames per stream.  With G the index of a frame in its stream since the reset (0, 1, ...),
after the decision::

    if speech:      every frame now in the line is flagged
    if G >= pre:    frame G - pre leaves the line; it is EMITTED iff its flag is set
    frame G enters the line with flag = keep

Equivalently ``keep'[g] = keep[g] or any(speech[g+1 .. g+pre])``: frame g is decided, and emitted if kept, while frame
g + pre is processed.  The gated stream G' is the concatenation of the emitted frames, copied bit for bit.  The newest ``pre``
frames of a stream are always undecided, and a push of n frames decides at most n, so a slot still gains at most one hop
per push.  Every emitted frame carries its source index g (``GatedScorer.last_span``): scores, verdict events and clips
count hops of the gated stream, and with look-ahead the emission also lags the input, so only the kernel that copies the
frames can say where in the call a scored hop came from.  ``reset`` drops the line.  A caller that wants the tail of a
finished call decided pushes one hop of zeros: zero frames are never speech, so they flag nothing.

Call tones (``ToneGate``; also stated in include/afx.h, afx_k_gate_tone).  The first seconds of a call are ringback, dial or
busy tone, IVR beeps, in-band DTMF, fax CNG / CED: loud, so the energy gate passes them as speech, and far outside anything
an anti-spoof model was trained on.  ``ToneGate(floor, ratio, rise, hang, frame, freqs=TELEPHONY_TONES, frac=0.85,
confirm=4, hold=3)`` is the plain gate (the first five parameters, the same checks, the same derived constants) plus a
Goertzel bank per frame at ``freqs`` (1 to 16 distinct frequencies in Hz, 0 < f < 8000; the gate works at 16 kHz).
``TELEPHONY_TONES`` is DTMF (697, 770, 852, 941, 1209, 1336, 1477, 1633), North American call progress (350, 440, 480, 620),
ETSI call progress (425), the 1004 Hz test tone, fax CNG (1100) and fax CED / echo-canceller disable (2100).  ``frac`` is a
finite fp32 number, 0 < frac <= 2; ``confirm`` >= 1 and ``hold`` >= 0 are frames.  Derived, each computed in float64 and
rounded to fp32 once on the host: ``c_k = fp32(2 cos(2 pi f_k / 16000))`` and ``thr = fp32(frac * frame / 2)``.  A sinusoid
of amplitude a over N samples has energy about a^2 N / 2 and Goertzel power about a^2 N^2 / 4, so ``T >= thr * e`` reads "at
least ``frac`` of the frame's energy sits at one or two bank frequencies".  Per stream the state is the plain gate's ``nf``
and ``h`` plus ``r`` (tonal frames in a row), ``q`` (hold frames left) and ``tones`` (tone frames since the reset), all 0 for
a new stream.  Every arithmetic operation is a single correctly rounded fp32 multiply, add or subtract (no fma).  Per frame,
in stream order::

    e, speech, the nf update:  exactly the plain gate's (same energy order, same operations)

    for every k:  s1 = s2 = +0.0
                  for i = 0 .. frame-1:   t = c_k * s1;  t = t - s2;  s0 = x[i] + t;  s2 = s1;  s1 = s0
                  a = s1 * s1;  b = s2 * s2;  m = c_k * s1;  m = m * s2;  P_k = (a + b) - m
    p1, p2 = the two largest of { P_k : P_k > +0.0 } as a multiset (a NaN or non-positive P_k counts as +0.0;
             fewer than two leave +0.0);   T = p1 + p2
    tonal  = (e < inf) and e > E_floor and T >= thr * e            (one fp32 multiply; false for any NaN)

    r = min(r + 1, 2^31 - 1) if tonal else 0
    if r >= confirm:  q = hold
    tone = r >= confirm or q > 0
    if r < confirm and q > 0:  q -= 1
    tones = min(tones + tone, 2^31 - 1)

    if tone:    speech = False;  h = 0          # a tone is not speech and ends the hangover
    if speech:  h = hang
    keep = speech or h > 0
    if not speech and h > 0:  h -= 1

Invariants: ``r >= confirm`` implies ``q == hold``, and ``0 <= q <= hold``.  The gated stream is the concatenation of the
kept frames, copied bit for bit, as for the plain gate.  Consequences: the first ``confirm - 1`` frames of a tone burst are
still decided as the plain gate decides them and may be kept -- the gate has no look-ahead; exactly ``hold`` frames after the
last confirmed frame are still tone, which bridges the beat nulls of 440 + 480 Hz ringback; a stream in which no frame is
ever ``tonal`` is gated exactly as ``SpeechGate`` with the same first five parameters gates it.  The defaults are
engineering defaults too, not tuned: there is no corpus in this repository.  ``ToneGate`` is not a ``LookaheadGate``:
tone rejection behind the delay line (which could also drop the first ``confirm - 1`` frames of a burst) is not built.

The contract of ``GatedScorer``: for a slot, let R be the concatenation of the hops it was pushed since its reset and G its
gated stream (G' with a ``LookaheadGate``; G as the function above defines it with a ``ToneGate``).  The slot's j-th non-NaN score equals, bit for bit, score j of a fresh inner
scorer of the same kind pushed G hop by hop, and it is emitted by the push in which sample ``(j + 1) * hop - 1`` of G was
kept (emitted from the delay line).  Nothing depends on the other slots, on the order or subsets in which slots are named,
or on session moves.  Behind a front, R is what that front's contract defines it to be.

The one read-back.  Which slots advance depends on the audio, so a push copies ``kept`` (one int32 per named slot) to pinned
host memory and waits for it: A x 4 bytes once per hop.  Everything else (ring heads, fills, counters) is host arithmetic
on that number.
"""
import math

import numpy as np
import torch

from ._layer import N_MAX, Layer, StreamState, _on, check_pending, export_pending, import_pending, need_gpu, rows_on, upload_pairs
from ._lib import AfxError, call_on, check, lib, ptr

GATE_FORMAT = 1  # layout of the gate part of a StreamState: import_slots refuses any other
MAX_FRAMES = 512  # frames of a row one afx_k_gate launch takes (the library splits longer rows itself)
MAX_TONES = 16  # frequencies of a ToneGate's bank (afx_k_gate_tone)
# the telephone network's signalling frequencies in Hz: DTMF rows and columns, North American call progress (dial, ringback,
# busy, reorder), ETSI call progress, the 1004 Hz test tone, fax CNG, fax CED / echo-canceller disable
TELEPHONY_TONES = (697, 770, 852, 941, 1209, 1336, 1477, 1633, 350, 440, 480, 620, 425, 1004, 1100, 2100)


def frame_energies(x, frame):
    """x: host fp32 array of whole frames -> (frames,) fp32, the energy of every frame in the order stated above."""
    f = np.ascontiguousarray(x, dtype=np.float32).reshape(-1, frame)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        sq = f * f
        p = np.zeros((f.shape[0], 64), dtype=np.float32)
        m = min(64, frame)
        p[:, :m] = sq[:, :m]
        for k in range(64, frame, 64):
            m = min(64, frame - k)
            p[:, :m] = p[:, :m] + sq[:, k:k + m]
        w = 32
        while w:
            p[:, :w] = p[:, :w] + p[:, w:2 * w]
            w //= 2
    return p[:, 0].copy()


def _number(name, v, integer=False):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer) if integer else (int, float, np.integer, np.floating)):
        raise ValueError(f"{name}: {'an integer' if integer else 'a number'}, got {v!r}")
    if not integer and not math.isfinite(v):
        raise ValueError(f"{name} must be finite, got {v!r}")
    return int(v) if integer else float(v)


class SpeechGate:
    """The gate's parameters and its offline form; see the module docstring for the function."""

    def __init__(self, floor=1e-6, ratio=8.0, rise=1.01, hang=20, frame=160):
        self.floor, self.ratio, self.rise = _number("floor", floor), _number("ratio", ratio), _number("rise", rise)
        self.hang, self.frame = _number("hang", hang, integer=True), _number("frame", frame, integer=True)
        if not self.floor > 0:
            raise ValueError(f"floor {floor!r}: a positive mean square per sample")
        if not self.ratio > 1:
            raise ValueError(f"ratio {ratio!r}: above 1")
        if not self.rise >= 1:
            raise ValueError(f"rise {rise!r}: at least 1")
        if self.hang < 0 or self.hang >= 1 << 31:
            raise ValueError(f"hang {hang!r}: a number of frames, 0 or more")
        if self.frame < 1 or self.frame >= 1 << 24:
            raise ValueError(f"frame {frame!r}: a positive number of samples")
        self.E_floor, self.ratio32, self.rise32 = np.float32(self.floor * self.frame), np.float32(self.ratio), np.float32(self.rise)
        if not (np.isfinite(self.E_floor) and self.E_floor > 0 and self.ratio32 > 1 and np.isfinite(self.ratio32) and
                np.isfinite(self.rise32)):
            raise ValueError("floor * frame, ratio and rise must be fp32 numbers (floor * frame > 0, ratio > 1)")
        self.nf_min = np.float32(self.E_floor / self.ratio32)  # one fp32 division

    def params(self):
        """What identifies this gate (plain ints and floats): two gates with equal params compute the same function."""
        return dict(floor=self.floor, ratio=self.ratio, rise=self.rise, hang=self.hang, frame=self.frame)

    @staticmethod
    def new_state():
        return {"nf": np.float32(np.inf), "h": 0}

    # ---- the numpy restatement -------------------------------------------------------------------------------------------
    def _frames(self, x):
        x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
        if x.size % self.frame:
            raise ValueError(f"{x.size} samples are not whole frames of {self.frame}")
        return x.reshape(-1, self.frame)

    def _decide(self, x, st, between=None):
        """The per-frame decision over x (whole frames) from the state st -> (frames (m, frame), speech, keep, nf, h).
        ``between(f, e, speech, h) -> (speech, h)`` is a form's own step on frame f of energy e, between the floor update
        and the hangover (the ``ToneGate``'s: the module docstring states that it belongs there)."""
        frames = self._frames(x)
        nf, h = np.float32(st["nf"]), int(st["h"])
        E_floor, ratio, rise, nf_min, inf = self.E_floor, self.ratio32, self.rise32, self.nf_min, np.float32(np.inf)
        e_all = frame_energies(frames, self.frame)
        speech, keep = np.zeros(e_all.size, dtype=bool), np.zeros(e_all.size, dtype=bool)
        with np.errstate(over="ignore", invalid="ignore", under="ignore"):
            for f, e in enumerate(e_all):
                fin = bool(e < inf)
                sp = fin and bool(e > max(E_floor, np.float32(ratio * nf)))
                if fin:
                    nf = max(nf_min, min(e, np.float32(nf * rise)))
                if between is not None:
                    sp, h = between(f, e, sp, h)
                if sp:
                    h = self.hang
                speech[f], keep[f] = sp, sp or h > 0
                if not sp and h > 0:
                    h -= 1
        return frames, speech, keep, np.float32(nf), h

    def gate_reference(self, x, state=None):
        """The function in numpy.  x: host fp32 array of whole frames (1-D, a multiple of ``frame`` samples); state: what an
        earlier call returned (None: a new stream; it is not modified) -> (keep_mask (frames,) bool, the kept samples, the
        state after x).  Chunked at any frame boundaries with the state carried it gives what the whole stream gives."""
        frames, _, keep, nf, h = self._decide(x, self.new_state() if state is None else state)
        return keep, frames[keep].reshape(-1).copy(), {"nf": nf, "h": h}

    # ---- the device form ---------------------------------------------------------------------------------------------------
    # What a form supplies to the offline form below and to ``GatedScorer``: the session keys it adds, the zero frames the
    # offline form appends, its per-slot device state beyond nf and h, its header, its launch and what it collects per clip.
    _session_keys = ()
    _pad = 0

    def _new_extra(self, S, ring_len, dev):
        """The form's device state beyond ``nf`` and ``h`` for S fresh slots with rings of ring_len samples (and the tables
        its launch reads) -> a dict of tensors; a ``GatedScorer`` shows them as attributes of these names."""
        return {}

    def _reset_extra(self, extra, rows):
        """Slots ``rows`` (a device index tensor) of the form's state become a new stream's."""

    def _header(self, slot, wpos, seen, dev):
        """-> the launch's header on ``dev``, without synchronisation: per row the slot, its ring's write position and
        whatever the form derives from the samples the slot has seen."""
        return upload_pairs(slot, wpos, dev)

    def _launch(self, x, hdr, nf, h, ring, kept, extra, mask=None):
        """afx_k_gate over the rows of x ((A, n) fp32 on the GPU, contiguous) with this gate's constants -> the form's
        by-product of a streamed push (``ToneGate``: the tone frames of each row; else None)."""
        check(call_on(x, lib().afx_k_gate, ptr(x), x.shape[0], x.shape[1], ptr(hdr), self.frame, float(self.E_floor),
                      float(self.ratio32), float(self.rise32), self.hang, ptr(nf), ptr(h), ptr(ring), ring.shape[0], ring.shape[1],
                      ptr(kept), ptr(mask)))

    def _collect(self, extra, mask, r, k):
        """-> what the offline form returns for row r beside its k kept samples (mask: (A, frames + _pad) uint8 or None)."""
        return () if mask is None else (mask[r].bool(),)

    def _offline(self, clips, want_mask, picks):
        """The offline form of every gate: the form's launch over whole clips, each with fresh state and ``_pad`` zero
        frames appended; one launch sequence and one read-back of the counts per distinct clip length (and 65535 clips).
        -> per pick j the list over the clips of entry j of (kept audio, *_collect(...)); a single pick: that list."""
        clips = list(clips.unbind(0)) if isinstance(clips, torch.Tensor) and clips.ndim == 2 else list(clips)
        for c in clips:
            if not isinstance(c, torch.Tensor) or c.ndim != 1 or c.dtype != torch.float32:
                raise ValueError("gate: a list of 1-D fp32 tensors or a (B, n) tensor")
            if not c.is_cuda:
                raise AfxError("the gate runs on the GPU; there is no CPU fallback (gate_reference is the numpy restatement)")
        got = [None] * len(clips)
        groups = {}
        for i, c in enumerate(clips):
            groups.setdefault((c.device, c.numel() // self.frame), []).append(i)
        for (dev, frames), rows in groups.items():
            n, total = frames * self.frame, frames + self._pad
            with torch.cuda.device(dev):
                for lo in range(0, len(rows), 65535):
                    part = rows[lo:lo + 65535]
                    A = len(part)
                    extra = self._new_extra(A, total * self.frame, dev)
                    mask = torch.zeros(A, total, dtype=torch.uint8, device=dev) if want_mask else None
                    ring = torch.empty(A, total * self.frame, dtype=torch.float32, device=dev)
                    kept = torch.zeros(A, dtype=torch.int32, device=dev)
                    if frames:  # (a clip without a whole frame: nothing to launch, nothing kept)
                        x = torch.stack([clips[i][:n] for i in part])
                        x = torch.nn.functional.pad(x, (0, self._pad * self.frame)) if self._pad else x.contiguous()
                        hdr = self._header(np.arange(A), np.zeros(A, dtype=np.int64), np.zeros(A, dtype=np.int64), dev)
                        nf = torch.full((A,), float("inf"), dtype=torch.float32, device=dev)
                        h = torch.zeros(A, dtype=torch.int32, device=dev)
                        self._launch(x, hdr, nf, h, ring, kept, extra, mask)
                    for r, (i, k) in enumerate(zip(part, kept.tolist())):
                        got[i] = (ring[r, :k].clone(),) + self._collect(extra, mask, r, k)
        res = tuple([g[j] for g in got] for j in picks)
        return res if len(res) > 1 else res[0]

    def gate(self, clips, return_mask=False):
        """The offline form: ``afx_k_gate`` over whole clips, each with fresh state.  clips: a list of 1-D CUDA fp32 tensors
        (any lengths) or a (B, n) CUDA tensor -> the list of kept-audio tensors (1-D, possibly empty), ready for
        ``model.forward_ragged``; with ``return_mask`` also the list of per-frame bool masks.  Trailing samples short of a
        whole frame are dropped.  One launch sequence and one read-back of the counts per distinct clip length."""
        return self._offline(clips, return_mask, (0, 1) if return_mask else (0,))


class LookaheadGate(SpeechGate):
    """The gate with ``pre`` frames of onset pre-roll by look-ahead (1 <= pre <= 31, default 5 = 50 ms); see the module
    docstring for the function.  ``GatedScorer(scorer, LookaheadGate(...))`` runs it streamed."""

    def __init__(self, floor=1e-6, ratio=8.0, rise=1.01, hang=20, frame=160, pre=5):
        super().__init__(floor, ratio, rise, hang, frame)
        self.pre = _number("pre", pre, integer=True)
        if not 1 <= self.pre <= 31:
            raise ValueError(f"pre {pre!r}: 1 to 31 frames of pre-roll")

    def params(self):
        return dict(super().params(), pre=self.pre)

    def new_state(self):
        """A new stream: the plain gate's state, an empty delay line (``line`` (d, frame) fp32, the d <= pre delayed
        frames, oldest first; ``flags`` (d,) bool) and ``F`` = 0 frames seen."""
        return {"nf": np.float32(np.inf), "h": 0, "line": np.zeros((0, self.frame), dtype=np.float32),
                "flags": np.zeros(0, dtype=bool), "F": 0}

    def gate_reference(self, x, state=None):
        """The function in numpy.  x: host fp32 array of whole frames; state: what an earlier call returned (None: a new
        stream; it is not modified) -> (keep' of the frames this chunk DECIDED, (decided,) bool: frames max(0, F - pre) ..
        F + frames - pre - 1 of the stream; the emitted samples; their source indices, int64; the state after x).
        Chunked at any frame boundaries with the state carried it gives what the whole stream gives."""
        st = self.new_state() if state is None else state
        frames, speech, keep, nf, h = self._decide(x, st)
        F, d = int(st["F"]), len(st["flags"])  # d = min(F, pre) frames are delayed
        both = np.concatenate([np.asarray(st["line"], dtype=np.float32).reshape(d, self.frame), frames])
        flags = np.concatenate([np.asarray(st["flags"], dtype=bool), keep])
        for j in np.flatnonzero(speech):  # chunk frame j sits at d + j: the line then holds the (up to) pre frames before it
            flags[max(0, d + j - self.pre):d + j] = True
        decided = max(0, d + frames.shape[0] - self.pre)
        mask = flags[:decided].copy()
        sources = (F - d + np.flatnonzero(mask)).astype(np.int64)
        new = {"nf": nf, "h": h, "line": both[decided:].copy(), "flags": flags[decided:].copy(), "F": F + frames.shape[0]}
        return mask, both[:decided][mask].reshape(-1).copy(), sources, new

    # ---- the device form ---------------------------------------------------------------------------------------------------
    _session_keys = ("gate_line", "gate_flags", "gate_sources")
    _pad = property(lambda self: self.pre)

    def _new_extra(self, S, ring_len, dev):
        return dict(flags=torch.zeros(S, dtype=torch.int32, device=dev),
                    line=torch.zeros(S, self.pre * self.frame, dtype=torch.float32, device=dev),
                    src=torch.full((S, ring_len // self.frame), -1, dtype=torch.int32, device=dev))

    def _reset_extra(self, extra, rows):
        extra["flags"][rows] = 0  # (the line's frames are then flagged by nobody and leave unemitted)
        extra["src"][rows] = -1

    def _header(self, slot, wpos, seen, dev):
        hdr = torch.zeros(len(slot), 4, dtype=torch.int32, pin_memory=True)
        hdr.numpy()[:, :3] = np.stack([slot, wpos, seen // self.frame], axis=1)  # F is host arithmetic
        return hdr.to(dev, non_blocking=True)

    def _launch(self, x, hdr, nf, h, ring, kept, extra, mask=None):
        """afx_k_gate_la over the rows of x ((A, n) fp32 on the GPU, contiguous; hdr (A, 4)) with this gate's constants."""
        check(call_on(x, lib().afx_k_gate_la, ptr(x), x.shape[0], x.shape[1], ptr(hdr), self.frame, float(self.E_floor),
                      float(self.ratio32), float(self.rise32), self.hang, self.pre, ptr(nf), ptr(h), ptr(extra["flags"]),
                      ptr(extra["line"]), ptr(ring), ptr(extra["src"]), ring.shape[0], ring.shape[1], ptr(kept), ptr(mask)))

    def _collect(self, extra, mask, r, k):
        sources = extra["src"][r, :k // self.frame].long()
        return (sources,) if mask is None else (sources, mask[r, self.pre:].bool())  # (mask entry j is the frame j - pre)

    def gate(self, clips, return_mask=False, return_sources=False):
        """The offline form: ``afx_k_gate_la`` over whole clips, each with fresh state and ``pre`` zero frames appended so
        that every real frame is decided (zero frames flag nothing and never leave the line).  clips as for
        ``SpeechGate.gate`` -> the list of gated-audio tensors; with ``return_mask`` also the list of per-frame bool masks
        (keep' of every real frame), with ``return_sources`` also the list of int64 tensors of the emitted frames' indices.
        Trailing samples short of a whole frame are dropped."""
        return self._offline(clips, return_mask, (0,) + ((2,) if return_mask else ()) + ((1,) if return_sources else ()))


class ToneGate(SpeechGate):
    """The gate that also rejects call tones: a Goertzel bank at ``freqs`` per frame, ``confirm`` tonal frames in a row make
    a tone, which lasts ``hold`` frames past the run; see the module docstring for the function.
    ``GatedScorer(scorer, ToneGate())`` runs it streamed."""

    def __init__(self, floor=1e-6, ratio=8.0, rise=1.01, hang=20, frame=160, freqs=TELEPHONY_TONES, frac=0.85, confirm=4, hold=3):
        super().__init__(floor, ratio, rise, hang, frame)
        if isinstance(freqs, (str, bytes)) or not isinstance(freqs, (tuple, list, np.ndarray)) or np.ndim(freqs) != 1:
            raise ValueError(f"freqs {freqs!r}: 1 to {MAX_TONES} frequencies in Hz")
        self.freqs = tuple(_number(f"freqs[{i}]", f) for i, f in enumerate(freqs))
        if not 1 <= len(self.freqs) <= MAX_TONES:
            raise ValueError(f"freqs: 1 to {MAX_TONES} frequencies, got {len(self.freqs)}")
        if len(set(self.freqs)) != len(self.freqs):
            raise ValueError(f"freqs {freqs!r}: a frequency is named twice")
        if not all(0 < f < 8000 for f in self.freqs):
            raise ValueError(f"freqs {freqs!r}: each above 0 and below 8000 Hz (the gate works at 16 kHz)")
        self.frac = _number("frac", frac)
        if not (0 < self.frac <= 2 and np.float32(self.frac) > 0):
            raise ValueError(f"frac {frac!r}: an fp32 number above 0, at most 2")
        self.confirm, self.hold = _number("confirm", confirm, integer=True), _number("hold", hold, integer=True)
        if self.confirm < 1 or self.confirm >= 1 << 31:
            raise ValueError(f"confirm {confirm!r}: a number of frames, 1 or more")
        if self.hold < 0 or self.hold >= 1 << 31:
            raise ValueError(f"hold {hold!r}: a number of frames, 0 or more")
        self.coef = np.array([2.0 * math.cos(2.0 * math.pi * f / 16000.0) for f in self.freqs], dtype=np.float64).astype(np.float32)
        self.thr = np.float32(self.frac * self.frame / 2)
        if not (np.isfinite(self.thr) and self.thr > 0):
            raise ValueError("frac * frame / 2 must be a positive fp32 number")

    def params(self):
        return dict(super().params(), freqs=list(self.freqs), frac=self.frac, confirm=self.confirm, hold=self.hold)

    @staticmethod
    def new_state():
        return {"nf": np.float32(np.inf), "h": 0, "r": 0, "q": 0, "tones": 0}

    # ---- the numpy restatement -------------------------------------------------------------------------------------------
    def tone_powers(self, x):
        """x: host fp32 array of whole frames -> (frames, K) fp32, the Goertzel power P_k of every frame at every bank
        frequency, in the operation order the module docstring states."""
        f = self._frames(x)
        c = self.coef[None, :]
        s1 = np.zeros((f.shape[0], c.shape[1]), dtype=np.float32)
        s2 = s1.copy()
        with np.errstate(all="ignore"):
            for i in range(self.frame):
                t = c * s1
                t = t - s2
                s0 = f[:, i, None] + t
                s2 = s1
                s1 = s0
            a, b = s1 * s1, s2 * s2
            m = c * s1
            m = m * s2
            return (a + b) - m

    def _tone_sums(self, x):
        """-> (frames,) fp32: T, the sum of the two largest positive powers of every frame."""
        P = self.tone_powers(x)
        with np.errstate(all="ignore"):
            v = np.sort(np.where(P > 0, P, np.float32(0.0)).astype(np.float32), axis=1)
            second = v[:, -2] if v.shape[1] > 1 else np.zeros(v.shape[0], dtype=np.float32)
            return (v[:, -1] + second).astype(np.float32)

    def _decide_tone(self, x, st):
        """The per-frame decision over x (whole frames) from the state st -> (frames (m, frame), T, tonal, tone, keep, the
        state after x)."""
        T_all = self._tone_sums(x)
        r, q, tones = int(st["r"]), int(st["q"]), int(st["tones"])
        top, inf = (1 << 31) - 1, np.float32(np.inf)
        tonal_all, tone_all = np.zeros(T_all.size, dtype=bool), np.zeros(T_all.size, dtype=bool)

        def between(f, e, speech, h):
            nonlocal r, q, tones
            tonal = bool(e < inf) and bool(e > self.E_floor) and bool(T_all[f] >= np.float32(self.thr * e))
            r = min(r + 1, top) if tonal else 0
            if r >= self.confirm:
                q = self.hold
            tone = r >= self.confirm or q > 0
            if r < self.confirm and q > 0:
                q -= 1
            tones = min(tones + tone, top)
            tonal_all[f], tone_all[f] = tonal, tone
            return (False, 0) if tone else (speech, h)  # a tone is not speech and ends the hangover

        frames, _, keep, nf, h = self._decide(x, st, between)
        return frames, T_all, tonal_all, tone_all, keep, {"nf": nf, "h": h, "r": r, "q": q, "tones": tones}

    def gate_reference(self, x, state=None):
        """The function in numpy.  x: host fp32 array of whole frames; state: what an earlier call returned (None: a new
        stream; it is not modified) -> (keep_mask (frames,) bool, the kept samples, the state after x).  Chunked at any
        frame boundaries with the state carried it gives what the whole stream gives."""
        frames, _, _, _, keep, new = self._decide_tone(x, self.new_state() if state is None else state)
        return keep, frames[keep].reshape(-1).copy(), new

    def decide_reference(self, x, state=None):
        """For tests and tuning: per frame of x (whole frames, from ``state``, None: a new stream) -> (T (frames,) fp32,
        tonal, tone, keep: (frames,) bool)."""
        return self._decide_tone(x, self.new_state() if state is None else state)[1:5]

    # ---- the device form ---------------------------------------------------------------------------------------------------
    _session_keys = ("gate_tone",)

    def _new_extra(self, S, ring_len, dev):
        return dict(coef=torch.from_numpy(self.coef.copy()).to(dev), tone_state=torch.zeros(S, 3, dtype=torch.int32, device=dev))

    def _reset_extra(self, extra, rows):
        extra["tone_state"][rows] = 0

    def _launch(self, x, hdr, nf, h, ring, kept, extra, mask=None):
        """afx_k_gate_tone over the rows of x ((A, n) fp32 on the GPU, contiguous) with this gate's constants -> (A,) int32
        on the device: the tone frames of each row."""
        coef, ntone = extra["coef"], torch.empty(x.shape[0], dtype=torch.int32, device=x.device)
        check(call_on(x, lib().afx_k_gate_tone, ptr(x), x.shape[0], x.shape[1], ptr(hdr), self.frame, float(self.E_floor),
                      float(self.ratio32), float(self.rise32), self.hang, ptr(coef), coef.numel(), float(self.thr), self.confirm,
                      self.hold, ptr(nf), ptr(h), ptr(extra["tone_state"]), ptr(ring), ring.shape[0], ring.shape[1], ptr(kept),
                      ptr(ntone), ptr(mask), None))
        return ntone

    def _collect(self, extra, mask, r, k):
        return () if mask is None else ((mask[r] & 1).bool(), (mask[r] & 2).bool())

    def gate(self, clips, return_mask=False, return_tones=False):
        """The offline form: ``afx_k_gate_tone`` over whole clips, each with fresh state.  clips as for ``SpeechGate.gate``
        -> the list of kept-audio tensors; with ``return_mask`` also the list of per-frame bool keep masks, with
        ``return_tones`` also the list of per-frame bool tone masks.  Trailing samples short of a whole frame are dropped.
        One launch sequence and one read-back of the counts per distinct clip length."""
        return self._offline(clips, return_mask or return_tones, (0,) + ((1,) if return_mask else ()) + ((2,) if return_tones else ()))


def emitted(scores):
    """``GatedScorer.push``'s result (or a FeedResult of a front around it) -> bool tensor: which entries are scores (a NaN
    stands for a push that completed no hop of speech)."""
    return ~torch.isnan(scores.scores if hasattr(scores, "scores") else scores)


# ---- the checks of a gate's part of a session, shared by the layers of kind "gate" (GatedScorer, afx.turns.TurnScorer) ------
def session_counts(t, keys, n):
    """The state tensors ``keys`` of ``t``, each (n,) int64 -> their host arrays."""
    counts = []
    for k in keys:
        c = t[k].cpu().reshape(-1)
        if c.dtype != torch.int64 or c.numel() != n:
            raise ValueError(f"import_slots: {k} is (n,) int64")
        counts.append(c.numpy())
    return counts


def check_floor_shape(nf, n):
    if tuple(nf.shape) != (n,) or nf.dtype != torch.float32:
        raise ValueError(f"import_slots: gate_nf {tuple(nf.shape)} {nf.dtype} is not {(n,)} float32")


def check_hang_and_floor(gate, hang, nf):
    if ((hang < 0) | (hang > gate.hang)).any():
        raise ValueError(f"import_slots: a session's hangover is outside 0..{gate.hang} frames")
    nf_host = nf.cpu()
    if bool(torch.isnan(nf_host).any()) or bool((nf_host < float(gate.nf_min)).any()):
        raise ValueError(f"import_slots: a session's noise floor is NaN or below the gate's minimum {float(gate.nf_min)!r}")


def check_tone(gate, t, n, seen):
    """The checks of ``gate_tone`` (a ``ToneGate``'s r, q, tones per session) -> (the tensor,)."""
    tone = t["gate_tone"]
    if tone.dtype != torch.int64 or tuple(tone.shape) != (n, 3):
        raise ValueError(f"import_slots: gate_tone is {(n, 3)} int64")
    r, q, tones = tone.cpu().numpy().T
    if (r < 0).any() or (r > N_MAX).any():
        raise ValueError("import_slots: a session's run of tonal frames is negative (or 2^31 or more)")
    if ((q < 0) | (q > gate.hold)).any():
        raise ValueError(f"import_slots: a session's tone hold is outside 0..{gate.hold} frames")
    if ((r >= gate.confirm) & (q != gate.hold)).any():
        raise ValueError("import_slots: a session inside a confirmed tone does not hold the full hold")
    if ((tones < 0) | (tones > seen // gate.frame)).any():
        raise ValueError("import_slots: a session counts more tone frames than it has seen frames (or fewer than 0)")
    return (tone,)


class GatedScorer(Layer):
    """``scorer`` (whatever stands below the gate in the stack order of ``afx._layer``; around a cascade, screen and
    verifier then see the same gated stream) behind a ``SpeechGate`` (default: the default gate); see the module docstring
    for the contract.  It presents the surface the fronts drive an inner scorer through, so it goes INSIDE them:
    ``PacketScorer(GatedScorer(inner), 8000, "mulaw")``.

    Per slot a ring of 2 hops of kept samples on the device (the fronts' pending ring with ``max_pending = 1``): a slot
    holds less than one hop before a push and gains at most one, so at most one hop pops.  Ring head and fill are the
    host's: the head moves only at pops, the fill grows by what the push's one read-back says was kept.

    Sessions: the part of a ``StreamState`` is ``gate_pending`` ((n, hop) fp32, the kept samples waiting, left-aligned,
    zeros after), ``gate_fill``, ``gate_hang``, ``gate_inner_seen`` ((n,) int64: pending samples, hangover frames left, the
    inner session's samples) and ``gate_nf`` ((n,) fp32), meta ``gate`` (format) and ``gate_params``; the state's ``seen``
    is the gate's ``samples_seen``.  Counters, a hangover or a noise floor that cannot be a gate's are refused.

    With a ``LookaheadGate`` the push launches ``afx_k_gate_la`` (state ``flags``, ``line``, ``src``; F = samples_seen /
    frame is host arithmetic) and sets ``last_span``: (A, 2) int64 on the device, in the row order of the newest push,
    [first source sample, one past the last source sample) of the hop that push completed, counted in the gate's input
    stream since the reset, and (-1, -1) where none completed -- read from ``src`` by device indexing, no synchronisation
    (with a plain gate it stays None).  A session's part then gains ``gate_line`` ((n, pre * frame) fp32, the delayed
    frames, oldest first, zero frames in front where fewer than ``pre`` are delayed), ``gate_flags`` ((n,) int64, bit j =
    the j-th oldest delayed frame's flag) and ``gate_sources`` ((n, hop / frame) int64, the pending frames' source
    indices, -1 after the fill); flags beyond the delayed frames and sources that are not strictly increasing below the
    oldest delayed frame are refused.  A plain-gate state and a look-ahead state refuse each other (``gate_params``).

    With a ``ToneGate`` the push launches ``afx_k_gate_tone`` (the coefficient table is uploaded once, at construction; state
    ``tone_state`` (S, 3) int32 = r, q, tones) -- still one gate launch, one read-back of A int32, one pop and one inner
    push.  ``tone_frames`` is the (S,) int32 view on the device of the tone frames since each slot's reset and
    ``last_tone_frames`` the (A,) int32 device tensor of the newest push's tone frames, in its row order (None with the
    other gates).  A session's part then gains ``gate_tone`` ((n, 3) int64: r, q, tones); a negative r, a q outside
    0..hold, ``r >= confirm`` with ``q != hold`` and a tones count that is negative or above the frames the session has seen
    are refused.  A tone state and a plain or look-ahead state refuse each other (``gate_params``, ``gate_tone``).

    Provenance (``afx.provenance``): a jitter front over a provenance layer attaches a plain or a tone gate on its way.  An
    attached gate takes the frame counts of the next push (``note_synthetic``), asks its gate launch for the mask (otherwise
    NULL, as ever), compacts the kept frames' counts into ``gsyn`` ((S, ring_len / frame) int32, ``afx_k_prov_compact``), sums
    a popped hop's entries (``afx_k_prov_take``) and notes them to what takes notes below; a session's part gains ``gate_syn``
    ((n, hop / frame) int64, the pending frames' counts, -1 after the fill).  Over a layer whose policy says ``through="all"``
    a look-ahead gate is attached too: it also owns ``gline`` ((S, pre) int32, the delayed frames' counts at block g mod pre,
    parallel to ``line``; ``reset`` leaves it alone), its push calls ``afx_k_prov_compact_la`` in the place of
    ``afx_k_prov_compact``, and a session's part also gains ``gate_syn_line`` ((n, pre) int64, laid out as ``gate_line``: the
    delayed frames' counts, oldest first, zeros in front).  A gate that is not attached does none of this."""

    layer = "gate"
    _keys = ("gate_pending", "gate_fill", "gate_hang", "gate_inner_seen", "gate_nf")
    _part = "speech-gate part (it was not exported by a GatedScorer)"
    _inner_seen = "gate_inner_seen"

    def __init__(self, scorer, gate=None):
        super().__init__(scorer)
        gate = SpeechGate() if gate is None else gate
        if not isinstance(gate, SpeechGate):
            raise ValueError("gate: a SpeechGate")
        if scorer.hop % gate.frame:
            raise ValueError(f"a hop of {scorer.hop} samples is not a whole number of {gate.frame}-sample frames")
        self.gate = gate
        self.ring_len = 2 * scorer.hop
        dev, S = scorer.device, scorer.S
        self.ring = torch.zeros(S, self.ring_len, dtype=torch.float32, device=dev)
        self.nf = torch.full((S,), float("inf"), dtype=torch.float32, device=dev)
        self.h = torch.zeros(S, dtype=torch.int32, device=dev)
        self._head = np.zeros(S, dtype=np.int64)  # ring position of each slot's oldest pending sample (host)
        self._fill = np.zeros(S, dtype=np.int64)  # pending kept samples per slot (host), always < hop between pushes
        self._seen = np.zeros(S, dtype=np.int64)  # samples pushed per slot since its reset (host)
        self._la = isinstance(gate, LookaheadGate)  # (which part a session carries; push notes last_span with look-ahead)
        self._tone = isinstance(gate, ToneGate)
        self.last_span = None
        self.last_tone_frames = None
        self._keys = GatedScorer._keys + gate._session_keys
        # the gate's own per-slot state, also as attributes: flags, line, src (look-ahead); coef, tone_state (tones)
        self._extra = gate._new_extra(S, self.ring_len, dev)
        for name, t in self._extra.items():
            setattr(self, name, t)
        self._syn = False  # (afx.provenance: a jitter front over a provenance layer attaches this gate)

    # ---- provenance (afx.provenance) ---------------------------------------------------------------------------------------
    def _attach_provenance(self):
        """A jitter front found a provenance layer below this gate: from now on the gate launch writes its mask, and ``gsyn``
        ((S, ring_len / frame) int32, parallel to the sample ring) holds the synthetic samples of every kept frame."""
        if not self._syn:
            from .provenance import note_target
            self._syn, self._syn_note, self._syn_below = True, None, note_target(self.scorer)
            self.gsyn = torch.zeros(self.S, self.ring_len // self.gate.frame, dtype=torch.int32, device=self.device)
            if self._la:  # the delayed frames' counts: frame g at block g mod pre, parallel to ``line``
                self.gline = torch.zeros(self.S, self.gate.pre, dtype=torch.int32, device=self.device)

    def note_synthetic(self, counts, slots):
        """counts: (A, hop / frame) int32 on the scorer's device, the synthetic samples of every frame of the hop the next
        ``push`` brings for each of ``slots`` (in its row order).  The next ``push`` must name exactly these slots; it
        consumes the note.  Only an attached gate takes notes."""
        if not self._syn:
            raise ValueError("this gate is not attached to a provenance layer (a jitter front over one attaches it)")
        idx = self._named(slots)
        shape = (len(idx), self.hop // self.gate.frame)
        if not isinstance(counts, torch.Tensor) or counts.dtype != torch.int32 or counts.shape != shape or counts.device != self.ring.device:
            raise ValueError(f"counts: an int32 tensor of shape {shape} on {self.ring.device}")
        self._syn_note = (idx, counts.contiguous())

    @property
    def samples_seen(self):
        """(S,) int64: the samples the gate was pushed per slot since its last ``reset`` (kept or not)."""
        return torch.from_numpy(self._seen.copy())

    @property
    def samples_kept(self):
        """(S,) int64: the samples the gate kept per slot: those the inner session has seen plus those pending."""
        return self.scorer.samples_seen + torch.from_numpy(self._fill)

    @property
    def pending(self):
        """(S,) int64: the kept samples waiting for their hop to fill, always < hop."""
        return torch.from_numpy(self._fill.copy())

    @property
    def tone_frames(self):
        """(S,) int32 view on the device: the tone frames a ``ToneGate`` rejected per slot since its reset (None with the
        other gates)."""
        return self.tone_state[:, 2] if self._tone else None

    emitted = staticmethod(emitted)

    def push(self, chunk, slots=None):
        """chunk: (A, hop) fp32 on the GPU, row i the next hop of slot slots[i] (None: every slot, in order) -> (A,) fp32 in
        the order named: the inner scorer's score where this push completed a hop of the slot's gated stream, NaN where it
        did not (that slot's inner session has not moved).  One ``afx_k_gate`` launch, one read-back of A int32 (see the
        module docstring), one ``afx_k_ingest_pop`` and one inner ``push`` over the ready slots."""
        idx = self._named(slots)
        dev, hop, A = self.device, self.hop, len(idx)
        need_gpu(dev, "hops are gated and scored")
        if not isinstance(chunk, torch.Tensor) or not chunk.is_cuda or chunk.dtype != torch.float32 or chunk.shape != (A, hop):
            raise ValueError(f"expected a CUDA fp32 tensor of shape {(A, hop)} (one hop per named slot)")
        la, frame = self._la, self.gate.frame
        note = None
        if self._syn:
            note, self._syn_note = self._syn_note, None
            if note is not None and note[0] != idx:
                raise ValueError(f"the note names the slots {note[0]}, this push {idx}: a note is for the next push of exactly its slots")
        if not A:
            if la:
                self.last_span = torch.empty(0, 2, dtype=torch.int64, device=dev)
            if self._tone:
                self.last_tone_frames = torch.empty(0, dtype=torch.int32, device=dev)
            return torch.empty(0, dtype=torch.float32, device=dev)
        slot = np.asarray(idx, dtype=np.int64)
        head, fill = self._head[slot], self._fill[slot]
        if la and (self._seen[slot] + hop >= frame << 31).any():
            raise ValueError("a slot has seen 2^31 frames since its reset: reset it")
        with torch.cuda.device(dev):
            kept = torch.empty(A, dtype=torch.int32, device=dev)
            hdr = self.gate._header(slot, (head + fill) % self.ring_len, self._seen[slot], dev)
            mask = torch.empty(A, hop // frame, dtype=torch.uint8, device=dev) if self._syn else None
            self.last_tone_frames = self.gate._launch(chunk.to(dev).contiguous(), hdr, self.nf, self.h, self.ring, kept, self._extra, mask)
            if self._syn:  # the kept frames' counts, in order, at the slot's write position in frames (hdr: the gate launch's own)
                counts = torch.zeros(A, hop // frame, dtype=torch.int32, device=dev) if note is None else note[1]
                if la:  # (the emitted frames' counts: out of gline, or the push's own, as the gate emits the samples)
                    check(call_on(self.gsyn, lib().afx_k_prov_compact_la, ptr(counts), ptr(mask), ptr(hdr), A, hop // frame, frame,
                                  self.gate.pre, ptr(self.gline), ptr(self.gsyn), self.S, self.ring_len // frame))
                else:
                    check(call_on(self.gsyn, lib().afx_k_prov_compact, ptr(counts), ptr(mask), ptr(hdr), A, hop // frame, frame,
                                  ptr(self.gsyn), self.S, self.ring_len // frame))
            if la:
                span = torch.full((A, 2), -1, dtype=torch.int64, device=dev)
            host = torch.empty(A, dtype=torch.int32, pin_memory=True)
            host.copy_(kept, non_blocking=True)
            torch.cuda.current_stream(dev).synchronize()  # the one read-back: which slots completed a hop is in the audio
            fill = fill + host.numpy()
            self._fill[slot] = fill
            self._seen[slot] += hop
            out = torch.full((A,), float("nan"), dtype=torch.float32, device=dev)
            rows = np.flatnonzero(fill >= hop)
            if rows.size:
                R = rows.size
                # the pop table (slot, head), then the result rows (look-ahead: and the src entries of each hop's ends)
                tab = torch.empty((5 if la else 3) * R, dtype=torch.int32, pin_memory=True)
                tab.numpy()[:2 * R] = np.stack([slot[rows], head[rows]], axis=1).reshape(-1)
                tab.numpy()[2 * R:3 * R] = rows
                if la:
                    tab.numpy()[3 * R:4 * R] = head[rows] // frame
                    tab.numpy()[4 * R:] = ((head[rows] + hop) // frame - 1) % (self.ring_len // frame)
                d = tab.to(dev, non_blocking=True)
                ready = torch.empty(R, hop, dtype=torch.float32, device=dev)
                check(call_on(self.ring, lib().afx_k_ingest_pop, ptr(self.ring), self.S, self.ring_len, ptr(d), R, hop, ptr(ready)))
                self._head[slot[rows]] = (head[rows] + hop) % self.ring_len
                self._fill[slot[rows]] = fill[rows] - hop
                if self._syn and self._syn_below is not None:  # the popped hops' sums, from the pop's own table
                    took = torch.empty(R, dtype=torch.int32, device=dev)
                    check(call_on(self.gsyn, lib().afx_k_prov_take, ptr(self.gsyn), self.S, self.ring_len // frame, ptr(d), R,
                                  hop // frame, frame, ptr(took)))
                    self._syn_below.note_synthetic(took, slot[rows].tolist())
                sc = self.scorer.push(ready, slot[rows].tolist())
                if sc is None:
                    raise RuntimeError("the inner scorer emitted no score for a hop")
                if R == A:
                    out = sc.to(torch.float32)
                else:
                    out.index_copy_(0, d[2 * R:3 * R].long(), sc.to(torch.float32))
                if la:
                    of = self.src[d[:2 * R:2].long()]  # (R, ring_len / frame): the popped slots' source indices
                    ends = torch.stack([of.gather(1, d[3 * R:4 * R].long()[:, None])[:, 0],
                                        of.gather(1, d[4 * R:].long()[:, None])[:, 0] + 1], dim=1)
                    span.index_copy_(0, d[2 * R:3 * R].long(), ends.long() * frame)
            if la:
                self.last_span = span
        return out

    def _reset(self, idx):
        """The noise floor (``nf = inf``), the hangover, the gate's own state, the pending samples and the counters are dropped."""
        if idx:
            with _on(self.device):
                rows = rows_on(idx, self.device)
                self.nf[rows] = float("inf")
                self.h[rows] = 0
                self.gate._reset_extra(self._extra, rows)
            self._head[idx] = 0
            self._fill[idx] = 0
            self._seen[idx] = 0

    # ---- sessions (afx._layer.Layer) -----------------------------------------------------------------------------------------
    def _meta(self):
        return dict(gate=GATE_FORMAT, gate_params=self.gate.params())

    def export_slots(self, slots):
        """``Layer.export_slots`` with the gate's own sample counts as the state's ``seen`` (the inner sessions' ride in
        ``gate_inner_seen``)."""
        st = super().export_slots(slots)
        return StreamState(st.meta, self._seen[self._slot_list(slots, ordered=True)], st.tensors)

    def _export(self, idx, st):
        with _on(self.device):
            rows = rows_on(idx, self.device)
            part = dict(gate_pending=export_pending(self.ring, idx, self._head[idx], self._fill[idx], self.hop),
                        gate_fill=torch.from_numpy(self._fill[idx]), gate_hang=self.h[rows].to("cpu", torch.int64),
                        gate_inner_seen=st.seen.clone(), gate_nf=self.nf[rows].clone())
            if self._la:
                part.update(self._export_line(idx, rows))
            if self._tone:
                part["gate_tone"] = self.tone_state[rows].to("cpu", torch.int64)
            if self._syn:  # the pending frames' synthetic samples, oldest first, -1 after the fill
                per = self.hop // self.gate.frame
                j = np.arange(per)
                ent = (self._head[idx][:, None] // self.gate.frame + j) % (self.ring_len // self.gate.frame)
                syn = self.gsyn[rows[:, None], torch.from_numpy(ent).to(self.device)].to("cpu", torch.int64)
                syn[torch.from_numpy(j[None, :] >= (self._fill[idx] // self.gate.frame)[:, None])] = -1
                part["gate_syn"] = syn
                if self._la:  # the delayed frames' counts, oldest first, zeros in front: gate_line's layout
                    pre = self.gate.pre
                    _, d, block = self._delayed(self._seen[idx])
                    ln = self.gline[rows[:, None], torch.from_numpy(block).to(self.device)].to("cpu", torch.int64)
                    ln[torch.from_numpy(np.arange(pre)[None, :] < (pre - d)[:, None])] = 0
                    part["gate_syn_line"] = ln
            return part

    def _state_keys(self, state):
        """``_keys``, and ``gate_syn`` (a look-ahead gate: and ``gate_syn_line``) where the state carries it: a state with
        the synthetic counts of its pending or delayed frames is refused by a gate that is not attached to a provenance
        layer, a state without them imports into an attached gate with zeros."""
        own = isinstance(state, StreamState)
        has, line = own and "gate_syn" in state.tensors, own and "gate_syn_line" in state.tensors
        if has and not self._syn:
            raise ValueError("import_slots: the state carries provenance counts (gate_syn) and this chain has no provenance layer")
        if line and not self._syn:
            raise ValueError("import_slots: the state carries provenance counts (gate_syn_line) and this chain has no provenance layer")
        return self._keys + (("gate_syn",) if has else ()) + (("gate_syn_line",) if line and self._la else ())

    def _delayed(self, seen):
        """seen: (n,) samples per session -> (F frames seen, d = min(F, pre) frames delayed, the line block of the exported
        block c (n, pre): exported block c holds frame F - pre + c, which sits at block (F + c) mod pre)."""
        F = np.asarray(seen, dtype=np.int64) // self.gate.frame
        return F, np.minimum(F, self.gate.pre), (F[:, None] + np.arange(self.gate.pre)) % self.gate.pre

    def _export_line(self, idx, rows):
        pre, frame, dev, n = self.gate.pre, self.gate.frame, self.device, len(idx)
        F, d, block = self._delayed(self._seen[idx])
        c = np.arange(pre)
        line = self.line.view(self.S, pre, frame)[rows[:, None], torch.from_numpy(block).to(dev)]
        line = line.masked_fill_(torch.from_numpy(c[None, :] < (pre - d)[:, None]).to(dev)[:, :, None], 0.0)
        dev_flags = self.flags[rows].cpu().numpy().astype(np.int64)
        bits = (dev_flags[:, None] >> block) & (c[None, :] >= (pre - d)[:, None])  # by exported block c; the j-th oldest is c = pre - d + j
        flags = np.array([sum(int(bits[i, pre - d[i] + j]) << j for j in range(d[i])) for i in range(n)], dtype=np.int64)
        per = self.hop // frame
        j = np.arange(per)
        ent = (self._head[idx][:, None] // frame + j) % (self.ring_len // frame)
        sources = self.src[rows[:, None], torch.from_numpy(ent).to(dev)].to("cpu", torch.int64)
        sources[torch.from_numpy(j[None, :] >= (self._fill[idx] // frame)[:, None])] = -1
        return dict(gate_line=line.reshape(n, pre * frame), gate_flags=torch.from_numpy(flags), gate_sources=sources)

    def _check(self, state, n):
        hop, t = self.hop, state.tensors
        fill, hang, inner_seen = session_counts(t, ("gate_fill", "gate_hang", "gate_inner_seen"), n)
        seen = state.seen.numpy()
        pend, nf = t["gate_pending"], t["gate_nf"]
        check_pending("gate_pending", pend, fill, n, hop)
        if pend.shape[1] != hop:
            raise ValueError(f"import_slots: gate_pending {tuple(pend.shape)} is not {(n, hop)}")
        check_floor_shape(nf, n)
        if ((fill >= hop) | (fill % self.gate.frame != 0)).any():
            raise ValueError(f"import_slots: a session's pending samples are not whole {self.gate.frame}-sample frames short of a hop")
        if ((inner_seen < 0) | (seen < 0) | (inner_seen % hop != 0) | (seen % hop != 0)).any():
            raise ValueError("import_slots: a session's sample count is not a whole number of hops")
        if (inner_seen + fill > seen).any():
            raise ValueError("import_slots: a session kept more samples than it was pushed")
        check_hang_and_floor(self.gate, hang, nf)
        syn = None  # (the pending frames' synthetic counts, where the state carries them: _state_keys)
        if "gate_syn" in t and self._syn:
            per, syn = hop // self.gate.frame, t["gate_syn"]
            if syn.dtype != torch.int64 or tuple(syn.shape) != (n, per):
                raise ValueError(f"import_slots: gate_syn is {(n, per)} int64")
            so = syn.cpu().numpy()
            pending = np.arange(per)[None, :] < (fill // self.gate.frame)[:, None]
            if (so[~pending] != -1).any() or (((so < 0) | (so > self.gate.frame)) & pending).any():
                raise ValueError(f"import_slots: gate_syn is 0..{self.gate.frame} for a session's pending frames and -1 after them")
        return (pend, nf, hang, fill, seen, syn) + (self._check_line(t, n, fill, seen) + (self._check_syn_line(t, n, seen),)
                                                    if self._la else ()) + (self._check_tone(t, n, seen) if self._tone else ())

    def _check_syn_line(self, t, n, seen):
        """``gate_syn_line`` where the state carries it and this gate is attached -> the tensor, else None."""
        if "gate_syn_line" not in t or not self._syn:
            return None
        pre, ln = self.gate.pre, t["gate_syn_line"]
        if ln.dtype != torch.int64 or tuple(ln.shape) != (n, pre):
            raise ValueError(f"import_slots: gate_syn_line is {(n, pre)} int64")
        lo = ln.cpu().numpy()
        _, d, _ = self._delayed(seen)
        delayed = np.arange(pre)[None, :] >= (pre - d)[:, None]
        if (lo[~delayed] != 0).any() or (((lo < 0) | (lo > self.gate.frame)) & delayed).any():
            raise ValueError(f"import_slots: gate_syn_line is 0..{self.gate.frame} for a session's delayed frames and 0 in front of them")
        return ln

    def _check_tone(self, t, n, seen):
        return check_tone(self.gate, t, n, seen)

    def _check_line(self, t, n, fill, seen):
        pre, frame, per = self.gate.pre, self.gate.frame, self.hop // self.gate.frame
        line, flags, sources = t["gate_line"], t["gate_flags"], t["gate_sources"]
        if tuple(line.shape) != (n, pre * frame) or line.dtype != torch.float32:
            raise ValueError(f"import_slots: gate_line {tuple(line.shape)} {line.dtype} is not {(n, pre * frame)} float32")
        if flags.dtype != torch.int64 or tuple(flags.shape) != (n,):
            raise ValueError("import_slots: gate_flags is (n,) int64")
        if sources.dtype != torch.int64 or tuple(sources.shape) != (n, per):
            raise ValueError(f"import_slots: gate_sources is {(n, per)} int64")
        F, d, block = self._delayed(seen)
        fl, so = flags.cpu().numpy(), sources.cpu().numpy()
        if ((fl < 0) | ((fl >> d) != 0)).any():
            raise ValueError("import_slots: a session flags a frame beyond those its delay line holds")
        pending = np.arange(per)[None, :] < (fill // frame)[:, None]
        if (so[~pending] != -1).any():
            raise ValueError("import_slots: gate_sources is -1 after a session's pending frames")
        if (((so < 0) | (so >= (F - d)[:, None])) & pending).any():
            raise ValueError("import_slots: a pending frame's source index is not below the session's oldest delayed frame")
        if ((np.diff(so, axis=1) <= 0) & pending[:, 1:]).any():
            raise ValueError("import_slots: a session's pending source indices are not strictly increasing")
        dev_flags = np.array([sum(((int(fl[i]) >> j) & 1) << int(block[i, pre - d[i] + j]) for j in range(d[i])) for i in range(n)],
                             dtype=np.int32)
        return line, dev_flags, block, sources

    def _import(self, idx, rows):
        pend, nf, hang, fill, seen, syn = rows[:6]
        if idx:
            import_pending(self.ring, idx, pend)
            with _on(self.device):
                dev_rows = rows_on(idx, self.device)
                self.nf[dev_rows] = nf.to(self.device)
                self.h[dev_rows] = torch.from_numpy(hang).to(self.device, torch.int32)
                if self._la:
                    line, dev_flags, block, sources, syn_line = rows[6:]
                    pre, frame, dev = self.gate.pre, self.gate.frame, self.device
                    self.line.view(self.S, pre, frame)[dev_rows[:, None], torch.from_numpy(block).to(dev)] = \
                        line.reshape(len(idx), pre, frame).to(dev)
                    if self._syn:
                        self.gline[dev_rows] = 0
                        if syn_line is not None:
                            self.gline[dev_rows[:, None], torch.from_numpy(block).to(dev)] = syn_line.to(dev, torch.int32)
                    self.flags[dev_rows] = torch.from_numpy(dev_flags).to(dev)
                    self.src[dev_rows] = -1
                    self.src[dev_rows, :sources.shape[1]] = sources.to(dev, torch.int32)
                if self._tone:
                    self.tone_state[dev_rows] = rows[6].to(self.device, torch.int32)
                if self._syn:
                    self.gsyn[dev_rows] = 0
                    if syn is not None:
                        self.gsyn[dev_rows, :syn.shape[1]] = syn.clamp(min=0).to(self.device, torch.int32)
            self._head[idx] = 0
            self._fill[idx] = fill
            self._seen[idx] = seen
