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
slots are named, or on session moves.  The end of a call is decided as for the gate: the caller pushes hops of zeros until
the hangover has run out.  Onset pre-roll (``LookaheadGate``) is not built for turns.

What the layers inside then mean: a verdict's hop index counts utterances; an evidence "hop" is a whole padded utterance;
the quality guard measures the padded clip, and its window count ``W`` is 1; a cascade's teacher re-scores a suspect
utterance.

The one read-back: which rows completed a turn is in the audio, so a push copies ``done`` (A x 16 bytes) to pinned host
memory and waits for it once -- in the place of ``GatedScorer``'s read-back of ``kept``.
"""
import numpy as np
import torch

from ._layer import N_MAX, Layer, StreamState, _on, integer, need_gpu, rows_on
from ._lib import call_on, check, lib, ptr
from .vad import GATE_FORMAT, LookaheadGate, SpeechGate, ToneGate, check_floor_shape, check_hang_and_floor, check_tone, emitted, session_counts

TURN_FORMAT = 1  # layout of the turn part of a StreamState: import_slots refuses any other
MAX_FRAMES = 512  # frames of a push (afx_k_turn's plan table)


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
    and -- if a row completed a turn -- one ``afx_k_turn_collect`` and one inner ``push`` over those rows.

    ``last_turn``: (A, 2) int64 on the device, in the row order of the newest push: [first source sample, one past the last)
    of the turn that push scored, (-1, -1) where it scored none; computed on the device from ``done``.  ``turn_totals``: the
    (S, 4) int32 device view of (scored, short, cut, kept).  ``stats()`` reads them back.

    Sessions: the part of a ``StreamState`` is ``gate_nf``, ``gate_hang``, ``gate_inner_seen`` (and ``gate_tone`` with a
    ``ToneGate``), laid out and checked as ``GatedScorer``'s; ``turn_open`` ((n, window) fp32: the open turn, left-aligned,
    zeros after), ``turn_frames`` and ``turn_first`` ((n,) int64; ``turn_first`` is -1 where ``turn_frames`` is 0) and
    ``turn_totals`` ((n, 4) int64); meta ``turn`` (format), ``turn_params`` = [hop, min_frames, max_frames], ``gate`` and
    ``gate_params``.  The state's ``seen`` is the layer's own sample count.  An imported open turn lands in buffer 0: which
    buffer holds it is not part of a session.  A ``GatedScorer`` state and a turn state refuse each other."""

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
            check(call_on(self.staging, lib().afx_k_turn, ptr(self.staging), self.S, hop, ptr(mask), ptr(th), A, self.F, frame,
                          self.min_frames, self.max_frames, ptr(self.bufs), ptr(self.turn_state), ptr(self._totals), ptr(done)))
            host = torch.empty(A, 4, dtype=torch.int32, pin_memory=True)
            host.copy_(done, non_blocking=True)
            wide = done.long()
            self.last_turn = torch.where(wide[:, 1:2] > 0, wide[:, 2:4] * frame, torch.full_like(wide[:, 2:4], -1))
            torch.cuda.current_stream(dev).synchronize()  # the one read-back: which rows closed a turn is in the audio
            d = host.numpy()
            if (d[:, 1] < 0).any():
                raise RuntimeError("afx_k_turn skipped a row: a slot's turn state is not a turn state")
            self._seen[slot] += hop
            out = torch.full((A,), float("nan"), dtype=torch.float32, device=dev)
            rows = np.flatnonzero(d[:, 1] > 0)
            if rows.size:
                R = rows.size
                tab = torch.empty(4 * R, dtype=torch.int32, pin_memory=True)  # the collect table (slot, buffer, frames), then the result rows
                tab.numpy()[:3 * R] = np.stack([slot[rows], d[rows, 0], d[rows, 1]], axis=1).reshape(-1)
                tab.numpy()[3 * R:] = rows
                t = tab.to(dev, non_blocking=True)
                clips = torch.empty(R, self.window, dtype=torch.float32, device=dev)
                check(call_on(self.bufs, lib().afx_k_turn_collect, ptr(self.bufs), self.S, self.max_frames, frame, ptr(t), R,
                              ptr(clips)))
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
            return part

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
        return (nf, hang, turn, frames, first, tot, seen) + (check_tone(self.gate, t, n, seen) if self._tone else ())

    def _import(self, idx, rows):
        nf, hang, turn, frames, first, tot, seen = rows[:7]
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
                    self.tone_state[dev_rows] = rows[7].to(dev, torch.int32)
            self._seen[idx] = seen
