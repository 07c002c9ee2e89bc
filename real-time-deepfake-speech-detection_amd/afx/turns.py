"""Talk spurts: score each turn of a call as one utterance.

The reference model is trained and evaluated per utterance: one clip, brought to the window by the reference's pad policy
(the clip repeated), gives one score.  ``GatedScorer`` concatenates the kept frames of a stream across talk spurts, so a
window mixes the end of one answer with the start of the next.  ``TurnScorer`` is a second layer of kind ``"gate"``: on the
GPU it cuts each slot's stream into turns (``afx_k_turn``), assembles the padded clip of every turn a push completes
(``afx_k_turn_collect``) and pushes those clips to the inner scorer, which must score exactly the clip it is pushed
(``scorer.hop == scorer.window``).

The function (also stated in include/afx.h, afx_k_turn / afx_k_turn_collect).  A *turn* is a maximal run of kept frames --
bit 0 of the gate's per-frame mask, hangover frames included -- cut when it reaches ``max_frames = window // frame``.
Parameters: ``min_frames`` (``TurnPolicy``, default 50 = 0.5 s), ``max_frames``, and the layer's own push size ``hop`` of
``F = hop // frame`` frames, ``F <= min_frames <= max_frames``.  State per slot, all 0 for a new stream: ``open`` (0 / 1:
which of the slot's two buffers collects the open turn), ``n`` (frames in the open turn, ``0 <= n < max_frames``), ``g`` (the
source index of the open turn's first frame) and ``totals = (scored, short, cut, kept)``, int32, each saturating at
2^31 - 1.  A push names rows of distinct slots; a row has F frames, ``g0 = samples_seen // frame`` before the push, and its
kept frames stand in order in the gate's staging ring.  Per row ``r = 0`` and ``done = (0, 0, 0, 0)``; for ``j = 0 .. F-1``
with ``G = g0 + j``::

    if mask[j] & 1:
        if n == 0: g = G
        buf[slot][open][n*frame .. (n+1)*frame) = staging frame r     (bit for bit);  r += 1; n += 1; kept += 1
        if n == max_frames: done = (open, n, g, G + 1); scored += 1; cut += 1; open ^= 1; n = 0
    elif n > 0:
        if n >= min_frames: done = (open, n, g, G); scored += 1; open ^= 1
        else:               short += 1
        n = 0

``done`` is (buffer, frames, first source frame, one past the last) of the turn the row completed.  A row whose ``g0`` is
negative or whose ``g0 + F`` reaches 2^31 is skipped whole with ``done = (-1, -1, -1, -1)``.  With ``F <= min_frames`` a row
completes at most one scored turn (after a close, fewer than F <= min_frames <= max_frames frames of the row remain), so the
buffer that is not ``open`` after the row holds the completed turn, or nothing of use, and the collect kernel reads it in the
same push: the whole reason for two buffers.  A turn shorter than ``min_frames`` is dropped and counted; the remainder of a
cut turn is a new turn and may be dropped the same way.  The clip of a scored turn of L samples is ``clip[k] = turn[k mod L]``,
``k < window``: ``afx_k_tile_crop``'s function with start 0, the reference's pad policy.  A cut turn is its own clip.

The contract of ``TurnScorer``.  Let ``T_0, T_1, ...`` be the scored turns of a slot in order and ``C_j`` their clips.  The
slot's j-th non-NaN score equals, bit for bit, score j of a fresh inner scorer of the same kind pushed ``C_0, C_1, ...``; with
a ``SlidingWindowScorer`` inside that is ``model.forward(C_j[None])[0, 1]``.  The score is returned by the push that brings
the frame that closes the turn -- the first non-kept frame, or the ``max_frames``-th kept one; every other push returns NaN
for the slot and the inner session does not move.  Nothing depends on the other slots, on the order or subsets in which
slots are named, or on session moves.  Onset pre-roll (``LookaheadGate``) is not built for turns.

The end of a call is the *close* step (``afx_k_turn_close``, ``TurnScorer.flush``), applied to ``(open, n, g, totals)``::

    if n >= min_frames:  done = (open, n, g, g + n); scored += 1; open ^= 1
    elif n > 0:          short += 1;                 done = (0, 0, 0, 0)
    else:                                            done = (0, 0, 0, 0)
    n = 0

``cut`` and ``kept`` do not move.  ``flush`` scores the turn that is open at hang-up at once and as it is: no hop of zeros
has to be pushed until the hangover runs out, and no frame of made-up silence joins the clip.

The offline form, ``score_turns``: a recording is the stream pushed hop by hop and then flushed.  The *cut* of a keep mask of
n frames is the recurrence above from a new stream's state over all n frames and then, with ``close_end``, the close step;
the scored turns are the ``done`` values with frames > 0 in stream order, each ``(first, end)`` in source frames with two
flags, ``cut`` (it closed by reaching ``max_frames``) and ``at_end`` (the close step closed it); short turns are counted,
not listed; without ``close_end`` the turn still open at the end is ``open = (first, frames)``, else ``(-1, 0)``.  A turn is
a run of kept frames, so its samples are contiguous in the source, ``x[first*frame : end*frame]``, and its clip is tiled
straight from the recording (``afx_k_turn_clips``): no staging ring and no buffers.  ``afx_k_turn_scan`` cuts the masks of
all recordings of a call in one go, ``SCAN_STEP`` frames a step per recording (include/afx.h states both).

What the layers inside then mean: a verdict's hop index counts utterances; an evidence "hop" is a whole padded utterance;
the quality guard measures the padded clip, and its window count ``W`` is 1; a cascade's teacher re-scores a suspect
utterance.

The one read-back: which rows completed a turn is in the audio, so a push copies ``done`` (A x 16 bytes) to pinned host
memory and waits for it once -- in the place of ``GatedScorer``'s read-back of ``kept``.
"""
import numpy as np
import torch

from ._layer import N_MAX, Layer, StreamState, _on, integer, need_gpu, rows_on
from ._lib import AfxError, call_on, check, lib, ptr
from .vad import GATE_FORMAT, LookaheadGate, SpeechGate, ToneGate, check_floor_shape, check_hang_and_floor, check_tone, emitted, session_counts

TURN_FORMAT = 1  # layout of the turn part of a StreamState: import_slots refuses any other
MAX_FRAMES = 512  # frames of a push (afx_k_turn's plan table)
SCAN_STEP = 4096  # frames a workgroup of afx_k_turn_scan takes per step: 256 threads x 16 mask bytes


def _count(v):
    return min(v + 1, N_MAX)


class TurnPolicy:
    """``min_frames``: the shortest turn that is scored, in frames of the gate (default 50 = 0.5 s at 10-ms frames); a shorter
    one is dropped and counted.  See the module docstring for the function; the two references restate it in numpy."""

    def __init__(self, min_frames=50):
        self.min_frames = integer("min_frames", min_frames, 1)

    @staticmethod
    def new_state(max_frames):
        """A new stream's state for turns of at most ``max_frames`` frames."""
        return {"open": 0, "n": 0, "g": 0, "totals": (0, 0, 0, 0), "max_frames": integer("max_frames", max_frames, 1)}

    def step_reference(self, state, mask_row, g0, kept=None, bufs=None):
        """One push of one slot on host mirrors.  state: ``new_state(max_frames)`` or what an earlier call returned (it is
        not modified); mask_row: (F,) the gate's mask bytes of the row; g0: the frames the slot has seen before it ->
        (the state after the row, done).  With ``kept`` ((r, frame) fp32: the row's kept frames in order) and ``bufs`` ((2,
        max_frames, frame) fp32, the slot's two buffers) the frames are copied as stated, in place."""
        mask_row = np.asarray(mask_row).reshape(-1)
        F, top = mask_row.size, state["max_frames"]
        if not self.min_frames <= top:
            raise ValueError(f"min_frames {self.min_frames} is above max_frames {top}")
        if g0 < 0 or g0 + F >= 1 << 31:
            return dict(state), (-1, -1, -1, -1)
        opn, n, g = state["open"], state["n"], state["g"]
        scored, short, cut, total = state["totals"]
        done, r = (0, 0, 0, 0), 0
        for j in range(F):
            G = g0 + j
            if int(mask_row[j]) & 1:
                if n == 0:
                    g = G
                if bufs is not None:
                    bufs[opn, n] = kept[r]
                r, n, total = r + 1, n + 1, _count(total)
                if n == top:
                    done = (opn, n, g, G + 1)
                    scored, cut, opn, n = _count(scored), _count(cut), opn ^ 1, 0
            elif n > 0:
                if n >= self.min_frames:
                    done = (opn, n, g, G)
                    scored, opn = _count(scored), opn ^ 1
                else:
                    short = _count(short)
                n = 0
        return {"open": opn, "n": n, "g": g, "totals": (scored, short, cut, total), "max_frames": top}, done

    def turns_reference(self, x, gate, max_frames=None):
        """A whole stream cut at once.  x: host fp32 array of whole frames (a new stream); gate: a ``SpeechGate`` or a
        ``ToneGate`` (its ``gate_reference`` gives the mask); max_frames: default 64000 // frame, the 4-s window ->
        (turns, totals, open): ``turns`` the closed runs in order, each a dict of ``first`` and ``end`` (source frames, end
        exclusive), ``close`` (the frame whose push returns the score: ``end`` for a natural end, ``end - 1`` for a cut),
        ``cut``, ``scored`` (False: dropped as short) and ``audio`` (its samples); ``totals`` = (scored, short, cut, kept);
        ``open`` = (first, frames) of the turn still open at the end of x, or None."""
        if isinstance(gate, LookaheadGate) or not isinstance(gate, SpeechGate):
            raise ValueError("gate: a SpeechGate or a ToneGate")
        top = 64000 // gate.frame if max_frames is None else integer("max_frames", max_frames, self.min_frames)
        keep = np.asarray(gate.gate_reference(x)[0], dtype=bool)
        frames = np.ascontiguousarray(x, dtype=np.float32).reshape(-1, gate.frame)
        turns, first = [], None
        for G in range(keep.size + 1):
            k = G < keep.size and bool(keep[G])
            n = 0 if first is None else G - first
            if first is not None and (not k or n == top):
                is_cut = n == top
                turns.append(dict(first=first, end=G, close=G - 1 if is_cut else G, cut=is_cut,
                                  scored=is_cut or n >= self.min_frames, audio=frames[first:G].reshape(-1).copy()))
                first = None
            if k and first is None:
                first = G
        if turns and turns[-1]["close"] >= keep.size:  # (the run reaches the end of x: it is still open)
            last = turns.pop()
            first = last["first"]
        scored = sum(t["scored"] for t in turns)
        kept_frames = int(keep.sum())
        totals = (scored, len(turns) - scored, sum(t["cut"] for t in turns), kept_frames)
        return turns, totals, (None if first is None else (first, keep.size - first))

    def close_reference(self, state):
        """The close step on a host mirror: the end of a call.  state: as for ``step_reference`` (it is not modified) -> (the
        state after it, done); the closed turn, if it is scored, stands in buffer ``done[0]`` as after a push."""
        opn, n, g = state["open"], state["n"], state["g"]
        scored, short, cut, total = state["totals"]
        done = (0, 0, 0, 0)
        if n >= self.min_frames:
            done = (opn, n, g, g + n)
            scored, opn = _count(scored), opn ^ 1
        elif n > 0:
            short = _count(short)
        return {"open": opn, "n": 0, "g": g, "totals": (scored, short, cut, total), "max_frames": state["max_frames"]}, done

    def cut_reference(self, keep, max_frames, close_end=True):
        """A whole stream cut at once, from its mask alone (the module docstring's *cut*).  keep: (n,) mask bytes or bools
        (bit 0 counts) -> (turns, totals, open): ``turns`` the scored turns in order, each a dict of ``first``, ``end``
        (source frames, end exclusive), ``cut`` and ``at_end``; ``totals`` = (scored, short, cut, kept); ``open`` = (first,
        frames) of the turn still open behind the last frame, (-1, 0) when there is none or with ``close_end``.  Stated as
        ``afx_k_turn_scan`` computes it, over whole arrays: frame G of a run that starts at s has position p = G - s; it
        closes a cut turn [G + 1 - max, G + 1) when (p + 1) % max == 0, else a natural turn [s + p // max * max, G + 1) of
        p % max + 1 frames when frame G + 1 is not kept (or is the end, with ``close_end``).  It equals ``step_reference``
        chained over pushes of any size, then ``close_reference``."""
        top = integer("max_frames", max_frames, self.min_frames)
        k = (np.asarray(keep).reshape(-1).astype(np.uint8) & 1).astype(bool)
        n = k.size
        if n >= 1 << 31:
            raise ValueError("a stream of 2^31 frames or more")
        idx = np.arange(n, dtype=np.int64)
        before = np.concatenate([[False], k[:-1]])
        after = np.concatenate([k[1:], [False]])
        s = np.maximum.accumulate(np.where(k & ~before, idx, -1)) if n else idx
        p = idx - s
        is_cut = k & ((p + 1) % top == 0)
        ends = k & ~is_cut & ~after
        if not close_end and n:
            ends[n - 1] = False
        length = p % top + 1
        is_scored = is_cut | (ends & (length >= self.min_frames))
        turns = [dict(first=int(G + 1 - top) if is_cut[G] else int(G + 1 - length[G]), end=int(G + 1), cut=bool(is_cut[G]),
                      at_end=bool(close_end and G == n - 1 and not is_cut[G])) for G in np.flatnonzero(is_scored)]
        totals = (int(is_scored.sum()), int((ends & ~is_scored).sum()), int(is_cut.sum()), int(k.sum()))
        still = (-1, 0)
        if n and not close_end and k[n - 1] and not is_cut[n - 1]:
            still = (int(n - length[n - 1]), int(length[n - 1]))
        return turns, totals, still

    @staticmethod
    def clip_reference(audio, window):
        """The padded clip of a turn: its samples repeated to ``window`` (``clip[k] = audio[k mod L]``)."""
        return np.resize(np.asarray(audio, dtype=np.float32), window)


class TurnScorer(Layer):
    """``scorer`` (whatever stands below the gate in the stack order of ``afx._layer``, with ``hop == window``: it scores the
    clip it is pushed) behind ``gate`` (a ``SpeechGate`` or a ``ToneGate``; default: the default ``SpeechGate``), cut into
    turns by ``policy`` (a ``TurnPolicy``); see the module docstring for the function and the contract.  ``hop`` is the
    layer's own push size, presented upward as ``.hop``; ``.window`` is the inner scorer's.  It goes where ``GatedScorer``
    goes, inside the fronts: ``PacketScorer(TurnScorer(inner), 8000, "mulaw")``.

    Per slot two buffers of one window on the device (2 x window x 4 bytes: 512 KB at 4 s) and a staging ring of one hop.
    A push is the gate's own launch into the staging ring (with its mask), one ``afx_k_turn``, the read-back of ``done``,
    and -- if a row completed a turn -- one ``afx_k_turn_collect`` and one inner ``push`` over those rows.  ``flush`` ends a
    call: the close step in the place of the gate's launch and ``afx_k_turn``, the rest the same.

    ``last_turn``: (A, 2) int64 on the device, in the row order of the newest push or flush: [first source sample, one past the last)
    of the turn that push scored, (-1, -1) where it scored none; computed on the device from ``done``.  ``turn_totals``: the
    (S, 4) int32 device view of (scored, short, cut, kept).  ``stats()`` reads them back.

    Sessions: the part of a ``StreamState`` is ``gate_nf``, ``gate_hang``, ``gate_inner_seen`` (and ``gate_tone`` with a
    ``ToneGate``), laid out and checked as ``GatedScorer``'s; ``turn_open`` ((n, window) fp32: the open turn, left-aligned,
    zeros after), ``turn_frames`` and ``turn_first`` ((n,) int64; ``turn_first`` is -1 where ``turn_frames`` is 0) and
    ``turn_totals`` ((n, 4) int64); meta ``turn`` (format), ``turn_params`` = [hop, min_frames, max_frames], ``gate`` and
    ``gate_params``.  The state's ``seen`` is the layer's own sample count.  An imported open turn lands in buffer 0: which
    buffer holds it is not part of a session.  A ``GatedScorer`` state and a turn state refuse each other.

    Provenance (``afx.provenance``): a jitter front over a provenance layer whose policy says ``through="all"`` attaches this
    layer.  It then takes the frame counts of the next push (``note_synthetic``, (A, hop / frame) int32), keeps ``bsyn`` ((S,
    2, max_frames) int32, parallel to ``bufs``: ``afx_k_prov_turn`` directly before ``afx_k_turn``), and the tail of ``push``
    and ``flush`` sums each scored turn's tiled count (``afx_k_prov_turn_sum`` beside the collect) and notes it to what takes
    notes below directly before the inner ``push``; ``done`` stays the one read-back.  A session's part gains ``turn_syn``
    ((n, max_frames) int64: the open turn's counts, then -1; it lands in buffer 0 with ``turn_open``).  A layer that is not
    attached does none of this."""

    layer = "gate"
    _keys = ("gate_nf", "gate_hang", "gate_inner_seen", "turn_open", "turn_frames", "turn_first", "turn_totals")
    _part = "turn part (it was not exported by a TurnScorer)"
    _inner_seen = "gate_inner_seen"

    def __init__(self, scorer, gate=None, policy=None, hop=4000):
        super().__init__(scorer)
        gate = SpeechGate() if gate is None else gate
        policy = TurnPolicy() if policy is None else policy
        if not isinstance(gate, SpeechGate):
            raise ValueError("gate: a SpeechGate or a ToneGate")
        if isinstance(gate, LookaheadGate):
            raise ValueError("gate: a SpeechGate or a ToneGate; onset pre-roll (LookaheadGate) is not built for turns")
        if not isinstance(policy, TurnPolicy):
            raise ValueError("policy: a TurnPolicy")
        if scorer.hop != scorer.window:
            raise ValueError(f"the inner scorer must score the clip it is pushed: hop == window, got hop {scorer.hop} and "
                             f"window {scorer.window} (a score is then a function of one turn alone)")
        frame = gate.frame
        if scorer.hop % frame:
            raise ValueError(f"a window of {scorer.hop} samples is not a whole number of {frame}-sample frames")
        hop = integer("hop", hop, 1)
        if hop % frame or not 1 <= hop // frame <= MAX_FRAMES:
            raise ValueError(f"hop {hop}: 1 to {MAX_FRAMES} whole frames of {frame} samples")
        self.gate, self.policy, self._hop = gate, policy, hop
        self.F, self.min_frames, self.max_frames = hop // frame, policy.min_frames, scorer.hop // frame
        if not self.F <= self.min_frames <= self.max_frames:
            raise ValueError(f"min_frames {self.min_frames}: at least the {self.F} frames of a push (a push then completes at "
                             f"most one scored turn) and at most the {self.max_frames} frames of the window")
        dev, S = scorer.device, scorer.S
        self.staging = torch.zeros(S, hop, dtype=torch.float32, device=dev)
        self.nf = torch.full((S,), float("inf"), dtype=torch.float32, device=dev)
        self.h = torch.zeros(S, dtype=torch.int32, device=dev)
        self.bufs = torch.zeros(S, 2, scorer.window, dtype=torch.float32, device=dev)
        self.turn_state = torch.zeros(S, 3, dtype=torch.int32, device=dev)  # open, n, g
        self._totals = torch.zeros(S, 4, dtype=torch.int32, device=dev)
        self._seen = np.zeros(S, dtype=np.int64)  # samples pushed per slot since its reset (host)
        self._tone = isinstance(gate, ToneGate)  # (the session then carries gate_tone)
        self.last_turn = None
        self.last_tone_frames = None
        self._keys = TurnScorer._keys + gate._session_keys
        self._extra = gate._new_extra(S, hop, dev)  # the gate's own per-slot state, also as attributes (coef, tone_state)
        for name, t in self._extra.items():
            setattr(self, name, t)
        self._syn = False  # (afx.provenance: a jitter front over a provenance layer with through="all" attaches this layer)

    # ---- provenance (afx.provenance) ---------------------------------------------------------------------------------------
    def _attach_provenance(self):
        """A jitter front found a provenance layer below this layer: from now on ``bsyn`` ((S, 2, max_frames) int32, parallel
        to ``bufs`` in frames) holds the synthetic samples of every frame of the open and the completed turns."""
        if not self._syn:
            from .provenance import note_target
            self._syn, self._syn_note, self._syn_below = True, None, note_target(self.scorer)
            self.bsyn = torch.zeros(self.S, 2, self.max_frames, dtype=torch.int32, device=self.device)

    def note_synthetic(self, counts, slots):
        """counts: (A, hop / frame) int32 on the scorer's device, the synthetic samples of every frame of the hop the next
        ``push`` brings for each of ``slots`` (in its row order).  The next ``push`` must name exactly these slots; it
        consumes the note (``flush`` neither takes nor consumes one).  Only an attached layer takes notes."""
        if not self._syn:
            raise ValueError("this layer is not attached to a provenance layer (a jitter front over one attaches it)")
        idx = self._named(slots)
        shape = (len(idx), self.F)
        if not isinstance(counts, torch.Tensor) or counts.dtype != torch.int32 or counts.shape != shape or counts.device != self.staging.device:
            raise ValueError(f"counts: an int32 tensor of shape {shape} on {self.staging.device}")
        self._syn_note = (idx, counts.contiguous())

    # ---- the surface ---------------------------------------------------------------------------------------------------------
    @property
    def hop(self):
        return self._hop

    @property
    def samples_seen(self):
        """(S,) int64: the samples the layer was pushed per slot since its last ``reset`` (kept or not)."""
        return torch.from_numpy(self._seen.copy())

    @property
    def turns_scored(self):
        """(S,) int64: the turns each slot's inner session has scored (its samples over the window)."""
        return self.scorer.samples_seen // self.window

    @property
    def turn_totals(self):
        """(S, 4) int32 view on the device: scored, short, cut turns and kept frames per slot since its reset."""
        return self._totals

    @property
    def tone_frames(self):
        """(S,) int32 view on the device: the tone frames a ``ToneGate`` rejected per slot (None with a plain gate)."""
        return self.tone_state[:, 2] if self._tone else None

    emitted = staticmethod(emitted)

    def stats(self):
        """-> dict of (S,) int64 host tensors ``scored``, ``short``, ``cut``, ``kept_frames`` (the totals) and ``open_frames``
        (the frames of each slot's open turn): the only read-back beside a push's ``done``."""
        tot, st = self._totals.cpu().long(), self.turn_state.cpu().long()
        return dict(scored=tot[:, 0], short=tot[:, 1], cut=tot[:, 2], kept_frames=tot[:, 3], open_frames=st[:, 1])

    def push(self, chunk, slots=None):
        """chunk: (A, hop) fp32 on the GPU, row i the next hop of slot slots[i] (None: every slot, in order) -> (A,) fp32 in
        the order named: the inner scorer's score of the turn this push closed, NaN where it closed none (that slot's inner
        session has not moved)."""
        idx = self._named(slots)
        dev, hop, A, frame = self.device, self._hop, len(idx), self.gate.frame
        need_gpu(dev, "turns are cut and scored")
        if not isinstance(chunk, torch.Tensor) or not chunk.is_cuda or chunk.dtype != torch.float32 or chunk.shape != (A, hop):
            raise ValueError(f"expected a CUDA fp32 tensor of shape {(A, hop)} (one hop per named slot)")
        note = None
        if self._syn:
            note, self._syn_note = self._syn_note, None
            if note is not None and note[0] != idx:
                raise ValueError(f"the note names the slots {note[0]}, this push {idx}: a note is for the next push of exactly its slots")
        if not A:
            self.last_turn = torch.empty(0, 2, dtype=torch.int64, device=dev)
            if self._tone:
                self.last_tone_frames = torch.empty(0, dtype=torch.int32, device=dev)
            return torch.empty(0, dtype=torch.float32, device=dev)
        slot = np.asarray(idx, dtype=np.int64)
        g0 = self._seen[slot] // frame
        if (g0 + self.F >= 1 << 31).any():
            raise ValueError("a slot has seen 2^31 frames since its reset: reset it")
        with torch.cuda.device(dev):
            zeros = np.zeros(A, dtype=np.int64)
            kept = torch.empty(A, dtype=torch.int32, device=dev)
            mask = torch.empty(A, self.F, dtype=torch.uint8, device=dev)
            done = torch.empty(A, 4, dtype=torch.int32, device=dev)
            hdr = self.gate._header(slot, zeros, self._seen[slot], dev)
            self.last_tone_frames = self.gate._launch(chunk.to(dev).contiguous(), hdr, self.nf, self.h, self.staging, kept,
                                                      self._extra, mask)
            th = torch.empty(A, 3, dtype=torch.int32, pin_memory=True)
            th.numpy()[:] = np.stack([slot, zeros, g0], axis=1)
            th = th.to(dev, non_blocking=True)
            if self._syn:  # the kept frames' counts go where afx_k_turn is about to put the frames (it reads the state: first)
                counts = torch.zeros(A, self.F, dtype=torch.int32, device=dev) if note is None else note[1]
                check(call_on(self.bsyn, lib().afx_k_prov_turn, ptr(counts), ptr(mask), ptr(th), A, self.F, frame, self.min_frames,
                              self.max_frames, ptr(self.turn_state), ptr(self.bsyn), self.S))
            check(call_on(self.staging, lib().afx_k_turn, ptr(self.staging), self.S, hop, ptr(mask), ptr(th), A, self.F, frame,
                          self.min_frames, self.max_frames, ptr(self.bufs), ptr(self.turn_state), ptr(self._totals), ptr(done)))
            d = self._read_done(done, "afx_k_turn")
            self._seen[slot] += hop
            return self._score_done(slot, d)

    def flush(self, slots=None):
        """The call has ended for the named slots (None: every slot, in order): the close step of the module docstring -> (A,)
        fp32 in the order named: the inner scorer's score of the turn that was open, as it is, NaN where none was or where
        it was shorter than ``min_frames`` (dropped and counted).  One ``afx_k_turn_close``, the read-back of ``done``, and
        -- where a row closed a scored turn -- ``afx_k_turn_collect`` and one inner ``push``, as in ``push``; ``last_turn``
        is set as a push sets it.  The score is bit for bit what the inner scorer gives the clip of the open turn.  The
        gate's state (noise floor, hangover, tone state) and ``samples_seen`` do not move: if the stream goes on, its next
        kept frame opens a new turn.  A second ``flush`` finds nothing open."""
        idx = self._named(slots)
        dev, A = self.device, len(idx)
        need_gpu(dev, "turns are cut and scored")
        if self._tone:
            self.last_tone_frames = torch.zeros(A, dtype=torch.int32, device=dev)
        if not A:
            self.last_turn = torch.empty(0, 2, dtype=torch.int64, device=dev)
            return torch.empty(0, dtype=torch.float32, device=dev)
        slot = np.asarray(idx, dtype=np.int64)
        with torch.cuda.device(dev):
            th = torch.empty(A, dtype=torch.int32, pin_memory=True)
            th.numpy()[:] = slot
            th = th.to(dev, non_blocking=True)
            done = torch.empty(A, 4, dtype=torch.int32, device=dev)
            check(call_on(self.turn_state, lib().afx_k_turn_close, ptr(th), A, self.S, self.min_frames, self.max_frames,
                          ptr(self.turn_state), ptr(self._totals), ptr(done)))
            return self._score_done(slot, self._read_done(done, "afx_k_turn_close"))

    def _read_done(self, done, who):
        """``done`` (A, 4) of a launch -> its host copy, with ``last_turn`` set from it on the device."""
        host = torch.empty(done.shape[0], 4, dtype=torch.int32, pin_memory=True)
        host.copy_(done, non_blocking=True)
        wide = done.long()
        self.last_turn = torch.where(wide[:, 1:2] > 0, wide[:, 2:4] * self.gate.frame, torch.full_like(wide[:, 2:4], -1))
        torch.cuda.current_stream(self.device).synchronize()  # the one read-back: which rows closed a turn is in the audio
        d = host.numpy()
        if (d[:, 1] < 0).any():
            raise RuntimeError(f"{who} skipped a row: a slot's turn state is not a turn state")
        return d

    def _score_done(self, slot, d):
        """The clips of the turns ``d`` names (rows of slots ``slot``), collected and pushed to the inner scorer -> (A,) fp32,
        NaN where a row completed no turn."""
        dev, A = self.device, len(slot)
        out = torch.full((A,), float("nan"), dtype=torch.float32, device=dev)
        rows = np.flatnonzero(d[:, 1] > 0)
        if rows.size:
            R = rows.size
            tab = torch.empty(4 * R, dtype=torch.int32, pin_memory=True)  # the collect table (slot, buffer, frames), then the result rows
            tab.numpy()[:3 * R] = np.stack([slot[rows], d[rows, 0], d[rows, 1]], axis=1).reshape(-1)
            tab.numpy()[3 * R:] = rows
            t = tab.to(dev, non_blocking=True)
            clips = torch.empty(R, self.window, dtype=torch.float32, device=dev)
            check(call_on(self.bufs, lib().afx_k_turn_collect, ptr(self.bufs), self.S, self.max_frames, self.gate.frame, ptr(t), R,
                          ptr(clips)))
            if self._syn and self._syn_below is not None:  # the tiled turns' counts, over the collect's own table
                c = torch.empty(R, dtype=torch.int32, device=dev)
                check(call_on(self.bsyn, lib().afx_k_prov_turn_sum, ptr(self.bsyn), self.S, self.max_frames, ptr(t), R, ptr(c)))
                self._syn_below.note_synthetic(c, slot[rows].tolist())
            sc = self.scorer.push(clips, slot[rows].tolist())
            if sc is None:
                raise RuntimeError("the inner scorer emitted no score for a turn")
            if R == A:
                out = sc.to(torch.float32)
            else:
                out.index_copy_(0, t[3 * R:].long(), sc.to(torch.float32))
        return out

    def _reset(self, idx):
        """The noise floor, the hangover, the gate's own state, the open turn and the totals are dropped."""
        if idx:
            with _on(self.device):
                rows = rows_on(idx, self.device)
                self.nf[rows] = float("inf")
                self.h[rows] = 0
                self.gate._reset_extra(self._extra, rows)
                self.turn_state[rows] = 0
                self._totals[rows] = 0
            self._seen[idx] = 0

    # ---- sessions (afx._layer.Layer) -----------------------------------------------------------------------------------------
    def _meta(self):
        return dict(turn=TURN_FORMAT, turn_params=[self._hop, self.min_frames, self.max_frames], gate=GATE_FORMAT,
                    gate_params=self.gate.params())

    def export_slots(self, slots):
        """``Layer.export_slots`` with the layer's own sample counts as the state's ``seen`` (the inner sessions' ride in
        ``gate_inner_seen``)."""
        st = super().export_slots(slots)
        return StreamState(st.meta, self._seen[self._slot_list(slots, ordered=True)], st.tensors)

    def _export(self, idx, st):
        with _on(self.device):
            rows = rows_on(idx, self.device)
            state = self.turn_state[rows].to("cpu", torch.int64)
            opn, n, g = state[:, 0], state[:, 1], state[:, 2]
            turn = self.bufs[rows, opn.to(self.device)]
            live = torch.arange(self.window)[None, :] < (n * self.gate.frame)[:, None]
            turn = turn.masked_fill_(~live.to(self.device), 0.0)
            part = dict(gate_nf=self.nf[rows].clone(), gate_hang=self.h[rows].to("cpu", torch.int64), gate_inner_seen=st.seen.clone(),
                        turn_open=turn, turn_frames=n.clone(), turn_first=torch.where(n > 0, g, torch.full_like(g, -1)),
                        turn_totals=self._totals[rows].to("cpu", torch.int64))
            if self._tone:
                part["gate_tone"] = self.tone_state[rows].to("cpu", torch.int64)
            if self._syn:  # the open turn's counts, -1 after its frames
                syn = self.bsyn[rows, opn.to(self.device)].to("cpu", torch.int64)
                syn[torch.arange(self.max_frames)[None, :] >= n[:, None]] = -1
                part["turn_syn"] = syn
            return part

    def _state_keys(self, state):
        """``_keys``, and ``turn_syn`` where the state carries it: a state with the synthetic counts of its open turn is
        refused by a layer that is not attached to a provenance layer, a state without them imports into an attached one
        with zeros."""
        has = isinstance(state, StreamState) and "turn_syn" in state.tensors
        if has and not self._syn:
            raise ValueError("import_slots: the state carries provenance counts (turn_syn) and this chain has no provenance layer")
        return self._keys + (("turn_syn",) if has else ())

    def _check(self, state, n):
        t, frame, window = state.tensors, self.gate.frame, self.window
        hang, inner_seen, frames, first = session_counts(t, ("gate_hang", "gate_inner_seen", "turn_frames", "turn_first"), n)
        seen = state.seen.numpy()
        nf, turn, totals = t["gate_nf"], t["turn_open"], t["turn_totals"]
        check_floor_shape(nf, n)
        if tuple(turn.shape) != (n, window) or turn.dtype != torch.float32:
            raise ValueError(f"import_slots: turn_open {tuple(turn.shape)} {turn.dtype} is not {(n, window)} float32")
        if tuple(totals.shape) != (n, 4) or totals.dtype != torch.int64:
            raise ValueError(f"import_slots: turn_totals is {(n, 4)} int64")
        if ((seen < 0) | (seen % self._hop != 0) | (inner_seen < 0) | (inner_seen % window != 0)).any():
            raise ValueError("import_slots: a session's sample count is not a whole number of hops (inside: of windows)")
        if (seen // frame + self.F >= 1 << 31).any():
            raise ValueError("import_slots: a session has seen 2^31 frames")
        if ((frames < 0) | (frames >= self.max_frames)).any():
            raise ValueError(f"import_slots: a session's open turn is outside 0..{self.max_frames - 1} frames")
        if (first[frames == 0] != -1).any() or (first[frames > 0] < 0).any():
            raise ValueError("import_slots: turn_first is the open turn's first source frame, -1 where no turn is open")
        if ((frames > 0) & (first + frames > seen // frame)).any():
            raise ValueError("import_slots: a session's open turn ends after the frames it has seen")
        after = torch.arange(window)[None, :] >= torch.from_numpy(frames * frame)[:, None]
        if bool(((turn.cpu() != 0) & after).any()):
            raise ValueError("import_slots: turn_open holds non-zero samples after a session's open turn")
        tot = totals.cpu().numpy()
        if ((tot < 0) | (tot > N_MAX)).any():
            raise ValueError("import_slots: a session's totals are negative (or 2^31 or more)")
        check_hang_and_floor(self.gate, hang, nf)
        syn = None  # (the open turn's synthetic counts, where the state carries them: _state_keys)
        if "turn_syn" in t and self._syn:
            syn = t["turn_syn"]
            if syn.dtype != torch.int64 or tuple(syn.shape) != (n, self.max_frames):
                raise ValueError(f"import_slots: turn_syn is {(n, self.max_frames)} int64")
            so = syn.cpu().numpy()
            live = np.arange(self.max_frames)[None, :] < frames[:, None]
            if (so[~live] != -1).any() or (((so < 0) | (so > frame)) & live).any():
                raise ValueError(f"import_slots: turn_syn is 0..{frame} for the frames of a session's open turn and -1 after them")
        return (nf, hang, turn, frames, first, tot, seen, syn) + (check_tone(self.gate, t, n, seen) if self._tone else ())

    def _import(self, idx, rows):
        nf, hang, turn, frames, first, tot, seen, syn = rows[:8]
        if idx:
            dev = self.device
            with _on(dev):
                dev_rows = rows_on(idx, dev)
                self.nf[dev_rows] = nf.to(dev)
                self.h[dev_rows] = torch.from_numpy(hang).to(dev, torch.int32)
                self.bufs[dev_rows, 0] = turn.to(dev)
                state = np.stack([np.zeros_like(frames), frames, np.maximum(first, 0)], axis=1)
                self.turn_state[dev_rows] = torch.from_numpy(state).to(dev, torch.int32)
                self._totals[dev_rows] = torch.from_numpy(tot).to(dev, torch.int32)
                if self._tone:
                    self.tone_state[dev_rows] = rows[8].to(dev, torch.int32)
                if self._syn:
                    self.bsyn[dev_rows] = 0
                    if syn is not None:
                        self.bsyn[dev_rows, 0] = syn.clamp(min=0).to(dev, torch.int32)
            self._seen[idx] = seen


# ---- the offline form ----------------------------------------------------------------------------------------------------------
class Turns:
    """The scored turns of one recording, in order: ``scores`` (n,) fp32 CPU, bonafide scores (class 1: low means spoof);
    ``starts`` / ``ends`` (n,) float64 bounds of each turn in input-rate samples (the resampler's delay taken out at other
    rates); ``cut`` / ``at_end`` (n,) bool: the turn closed by reaching the window / by the end of the recording; ``totals``:
    a dict of ``scored``, ``short``, ``cut``, ``kept_frames`` and ``open_frames`` (the frames of the turn still open at the
    end: 0 with ``close_end``); ``sample_rate`` the input rate."""

    def __init__(self, scores, starts, ends, cut, at_end, totals=None, sample_rate=16000):
        self.scores = torch.as_tensor(scores, dtype=torch.float32).cpu().reshape(-1)
        self.starts = torch.as_tensor(starts, dtype=torch.float64).cpu().reshape(-1)
        self.ends = torch.as_tensor(ends, dtype=torch.float64).cpu().reshape(-1)
        self.cut = torch.as_tensor(cut, dtype=torch.bool).cpu().reshape(-1)
        self.at_end = torch.as_tensor(at_end, dtype=torch.bool).cpu().reshape(-1)
        self.totals = dict(scored=len(self), short=0, cut=int(self.cut.sum()), kept_frames=0, open_frames=0) if totals is None else dict(totals)
        self.sample_rate = int(sample_rate)
        if not self.scores.numel() == self.starts.numel() == self.ends.numel() == self.cut.numel() == self.at_end.numel():
            raise ValueError("scores, starts, ends, cut and at_end differ in length")

    def __len__(self):
        return int(self.scores.numel())

    def times(self):
        """(n, 2) float64: each turn's (start, end) in seconds."""
        return torch.stack([self.starts, self.ends], dim=1) / self.sample_rate

    def segments(self, threshold):
        """The (start_s, end_s) of the turns scoring below ``threshold``; the pieces of one run of speech that the window cut
        (a turn that begins where the one before it ends) are merged when both score below it."""
        out, last = [], None  # last: where the turn before this one ended, if it scored below the threshold
        for s, e, low in zip(self.starts.tolist(), self.ends.tolist(), (self.scores < threshold).tolist()):
            if low and s == last:
                out[-1] = (out[-1][0], e / self.sample_rate)
            elif low:
                out.append((s / self.sample_rate, e / self.sample_rate))
            last = e if low else None
        return out

    def alarms(self, policy):
        """The alarms a ``VerdictPolicy`` raises over these turns (``policy.run_reference`` over ``scores``, the hop index
        counting utterances 1, 2, ...: what a ``VerdictScorer`` inside a one-slot ``TurnScorer`` logs): a list of
        ``(raised_s, cleared_s or None, kind)`` -- the ends, in seconds, of the turns at which the alarm was raised and
        cleared (None: still on at the end), and the raise's kind."""
        events, _ = policy.run_reference(self.scores.numpy())
        ends = (self.ends / self.sample_rate).tolist()
        out = []
        for _slot, kind, j, _bits in events:
            if kind == 3:
                out[-1] = (out[-1][0], ends[j - 1], out[-1][2])
            else:
                out.append((ends[j - 1], None, kind))
        return out

    def summary(self, threshold):
        """The number of turns, min, mean and the fraction of turns scoring below ``threshold`` (flagged as spoof)."""
        n = len(self)
        if n == 0:
            return {"turns": 0, "min": float("nan"), "mean": float("nan"), "flagged": 0.0}
        return {"turns": n, "min": float(self.scores.min()), "mean": float(self.scores.double().mean()),
                "flagged": float((self.scores < threshold).double().mean())}


_stage = None  # a callable(name) that is told where each stage of score_turns begins (tools/turn_bench.py times them)


def _mark(name):
    if _stage is not None:
        _stage(name)


def score_turns(model, recordings, gate=None, policy=None, window=64000, sample_rate=16000, close_end=True, batch=None,
                state_dict=None):
    """Score every talk spurt of recorded calls as one utterance (the module docstring's offline form) -> one ``Turns`` per
    recording; a recording with no scored turn yields an empty one.

    model: an afx ``Engine`` (``state_dict`` is accepted as for ``score_timeline``), or a drop-in ``models.*`` module.
    recordings: a list of 1-D waveforms of any lengths at ``sample_rate``, on the host or on the GPU; trailing samples short
    of a frame are dropped, as in ``gate()``.  gate: a ``SpeechGate`` or a ``ToneGate`` (default: the default
    ``SpeechGate``); policy: a ``TurnPolicy``; window: the clip length the model scores, whole frames; ``close_end``: the end
    of a recording is the end of the call (False: the turn open there is not scored and is reported in ``totals``).  At
    another sample rate the recordings are resampled first (``Resampler.clips``) and the spans mapped back.

    The gate's offline launch gives the keep masks; one ``afx_k_turn_scan`` cuts them all, one read-back says how many turns
    there are, and per batch of at most ``batch`` turns (default: ``timeline.default_batch``) one ``afx_k_turn_clips`` tiles
    the clips from the recordings and ``Engine.forward`` scores them.  Contract: turn j of recording i has the spans of
    ``cut_reference`` on that recording's mask, its score is bit for bit ``model.forward(clip[None])[0, 1]``, and for a
    recording of whole hops the scores are, in order, the non-NaN scores of one slot of a ``TurnScorer`` over a
    ``SlidingWindowScorer(model, S, window, window)`` pushed the recording hop by hop and then flushed."""
    from .timeline import _resolve, default_batch
    eng, _ = _resolve(model, state_dict)
    gate = SpeechGate() if gate is None else gate
    policy = TurnPolicy() if policy is None else policy
    if not isinstance(gate, SpeechGate):
        raise ValueError("gate: a SpeechGate or a ToneGate")
    if isinstance(gate, LookaheadGate):
        raise ValueError("gate: a SpeechGate or a ToneGate; onset pre-roll (LookaheadGate) is not built for turns")
    if not isinstance(policy, TurnPolicy):
        raise ValueError("policy: a TurnPolicy")
    window, frame, least = integer("window", window, 1, 1 << 30), gate.frame, policy.min_frames
    if window % frame:
        raise ValueError(f"a window of {window} samples is not a whole number of {frame}-sample frames")
    top = window // frame
    if least > top:
        raise ValueError(f"min_frames {least}: at most the {top} frames of the window")
    recs = [torch.as_tensor(x).reshape(-1) for x in recordings]
    if len(recs) > 65535:
        raise ValueError("at most 65535 recordings a call")
    batch = default_batch(eng) if batch is None else integer("batch", batch, 1, 65535)
    if not torch.cuda.is_available():
        raise AfxError("turns are cut and scored on the GPU; there is no CPU fallback")
    dev = torch.device(eng.device)
    rate, delay = 16000, 0.0
    with torch.cuda.device(dev):
        if sample_rate != 16000:
            from .resample import Resampler
            rs = Resampler(sample_rate, dev)
            rate, delay = rs.rate, rs.delay
            recs = rs.clips([x.to(dev) for x in recs])
        recs = [x.to(dev, torch.float32) for x in recs]
        A = len(recs)
        if not A:
            return []
        _mark("gate")
        masks = gate.gate(recs, return_mask=True)[1]
        _mark("scan")
        n = np.array([m.numel() for m in masks], dtype=np.int64)
        cap = int((n // least).sum())  # (a scored turn has at least min_frames frames)
        hdr = torch.empty(2, A + 1, dtype=torch.int64, pin_memory=True)  # frame offsets, sample offsets
        hdr.numpy()[0, 0], hdr.numpy()[0, 1:] = 0, np.cumsum(n)
        hdr.numpy()[1] = hdr.numpy()[0] * frame
        hdr = hdr.to(dev, non_blocking=True)
        c4 = 4 * max(cap, 1)

        def parts(t):  # the scan's outputs stand in one buffer, for one copy to the host: table, row_base, totals, open
            return t[:c4].view(-1, 4), t[c4:c4 + A + 1], t[c4 + A + 1:c4 + 5 * A + 1].view(A, 4), t[c4 + 5 * A + 1:].view(A, 2)

        ints = torch.zeros(c4 + 7 * A + 1, dtype=torch.int32, device=dev)
        table, row_base, totals, still = parts(ints)
        R = 0
        if int(n.sum()):
            mask = torch.cat([m.to(torch.uint8) for m in masks])
            check(call_on(mask, lib().afx_k_turn_scan, ptr(mask), ptr(hdr[0]), A, least, top, int(bool(close_end)), ptr(table),
                          cap, ptr(row_base), ptr(totals), ptr(still)))
            R = int(row_base[A])  # the one read-back before the clips: how many turns there are
            if R > cap:
                raise RuntimeError(f"afx_k_turn_scan counted {R} turns where at most {cap} fit")
        else:
            still[:, 0] = -1
        scores = torch.empty(R, dtype=torch.float32, device=dev)
        if R:
            x = torch.cat([r[:k * frame] for r, k in zip(recs, n.tolist())])
            for r0 in range(0, R, batch):
                Rb = min(batch, R - r0)
                _mark("clips")
                clips = torch.empty(Rb, window, dtype=torch.float32, device=dev)
                check(call_on(x, lib().afx_k_turn_clips, ptr(x), ptr(hdr[1]), A, frame, top, ptr(table), r0, Rb, ptr(clips)))
                _mark("forward")
                scores[r0:r0 + Rb] = eng.forward(clips)[:, 1]
        _mark("end")
        table, base, totals, still = parts(ints.cpu())
        scores = scores.cpu()
    table, base, totals, still = table[:R], base.tolist(), totals.tolist(), still.tolist()
    scale = rate / 16000.0
    out = []
    for i in range(A):
        t = table[base[i]:base[i + 1]]
        st, en = t[:, 1].double() * frame, t[:, 2].double() * frame
        if delay:  # 16 kHz sample k of the resampled stream is input time (k - delay) / 16000 s
            st, en = (st - delay).clamp(min=0), (en - delay).clamp(min=0)
        tot = dict(scored=totals[i][0], short=totals[i][1], cut=totals[i][2], kept_frames=totals[i][3], open_frames=still[i][1])
        out.append(Turns(scores[base[i]:base[i + 1]], st * scale, en * scale, (t[:, 3] & 1).bool(), (t[:, 3] & 2).bool(), tot, rate))
    return out
