"""Evidence clips on the GPU: the audio the model judged and the scores that led up to an alarm, captured around every raise
of a ``VerdictScorer`` and read back once, at the caller's leisure.

``EvidenceScorer(VerdictScorer(...), policy)`` keeps, per slot, a pre-roll ring of the hops pushed to the inner scorer and of
their scores, and a small pool of clips.  The push that raises a slot's alarm opens a clip with the pre-roll and the raising
hop; the following pushes of that slot append the post-roll.  Everything stays on the device: a push adds one pinned upload
and two launches (``afx_k_evidence_mark``, ``afx_k_evidence_copy``) and no synchronisation, and ``take_clips()`` is the only
read-back.  Behind a gate or a jitter buffer the clip is the stream the model saw: the gated, concealed hops, which exist
on the device only.  ``Evidence(S, policy, hop, device)`` is the state and the pool on their own.

The function (also stated in include/afx.h).  ``EvidencePolicy(pre, post, clips, encoding)``: ``pre`` hops kept before the
raising hop (None: ``window // hop - 1``, so that a clip opens with exactly the window that raised the alarm), ``post`` hops
after it, ``clips`` pool entries, ``encoding`` "fp32" (samples bit for bit) or "pcm16".  P = pre + 1; a clip holds
L = P + post hops.  Per slot on the device: ``hist`` (S, P hop) fp32, the audio ring; ``sring`` (S, P) fp32, the score ring;
``rec`` (S,) int32, the pool entry being recorded or -1; ``left`` (S,) int32, the post-roll hops still to append.  The pool:
``pool`` (clips, 6) int32 headers ``(status, slot, raised_at, first_hop, hops, seq)`` with status 0 FREE, 1 RECORDING,
2 COMPLETE, 3 TRUNCATED; ``audio`` (clips, L hop) fp32 or int16; ``cscores`` (clips, L) fp32; ``counters`` (4,) int32 =
``raised, recorded, dropped, merged``.

An update names rows i = 0..A-1: a slot b_i (distinct), its hop of ``hop`` fp32 samples, its 1-based hop number k_i (int32:
the host's ``samples_seen // hop`` after this hop), its score s_i (fp32, NaN if this push produced none) and the verdict
state row ``(n, run, on, since)`` of the slot, read on the device after this push's verdict update.  The update behaves as if
the rows were processed in ascending row position::

    store:  hist[b][((k-1) hop + j) mod (P hop)] = sample j of the hop;  sring[b][(k-1) mod P] = s_i
    raise = on == 1 and since == k                  # raised by this very push: no extra state detects it
    if rec[b] >= 0:                                 # recording
        merged += raise                             # a raise while recording opens no second clip
        e = rec[b]; the hop, encoded, and s_i go to position hops_e of clip e; hops_e += 1; left[b] -= 1
        if left[b] == 0: status_e = COMPLETE; rec[b] = -1
    elif raise:
        raised += 1
        e = the FREE entry of lowest index not yet taken by an earlier row of this update
        if there is none: dropped += 1, and nothing else happens
        f = max(1, k - pre)
        header_e = (COMPLETE if post == 0 else RECORDING, b, k, f, k - f + 1, seq = recorded); recorded += 1
        hops f..k are read out of the ring (which already holds hop k), encoded into positions 0.., with their scores
        if post > 0: rec[b] = e; left[b] = post

Entries become FREE only in ``take_clips()``, between updates, so the free set is fixed during an update and allocation is a
prefix count of the raising rows into the ascending list of free entries: deterministic whatever the launch geometry.
``f = max(1, k - pre)``: a ring that still holds a previous session's samples is never read after a reset.  "pcm16" of a
sample x: ``q = x * 32768`` is one fp32 multiply, NaN becomes 0, q is clamped to [-32768, 32767] and rounded half to even
(``np.rint``), then stored as int16.  ``reset(slots)`` marks a clip being recorded by a named slot TRUNCATED: the clip is
kept with the hops it has, ``rec = -1``, ``left = 0``.

``EvidencePolicy.step_reference`` restates one update in numpy on host mirrors of all of the above (``new_state``),
``run_reference`` drives it over whole streams row by row; the kernels are bit-exact to it (tests/test_gpu_evidence.py).
"""
import wave

import numpy as np
import torch

from ._layer import N_MAX, Field, Layer, SlotTable, _on, hop_indices, integer, need_gpu, returned_scores, slot_count, slots_of, upload_pairs
from ._lib import call_on, check, lib, ptr

EVIDENCE_FORMAT = 1  # layout of the evidence part of a StreamState: import_slots refuses any other
MAX_CLIPS = 8192     # pool entries (the free list of afx_k_evidence_mark lives in LDS)
MAX_HOPS = 65535     # pre and post
FREE, RECORDING, COMPLETE, TRUNCATED = 0, 1, 2, 3
ENCODINGS = ("fp32", "pcm16")


def pcm16_reference(x):
    """The "pcm16" encoding of fp32 samples in numpy: one fp32 multiply by 32768, NaN -> 0, clamped to [-32768, 32767],
    rounded half to even -> int16."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        q = x * np.float32(32768)
        q = np.where(np.isnan(q), np.float32(0), q)
        q = np.rint(np.clip(q, np.float32(-32768), np.float32(32767)))
    return q.astype(np.int16)


class Clip:
    """One evidence clip on the host: ``slot``, ``raised_at`` (the hop number of the raising hop), ``first_hop`` (the hop
    number of the clip's first hop: the raising hop sits at position ``raised_at - first_hop``), ``audio`` ((hops * hop,)
    float32 or int16), ``scores`` ((hops,) float32, NaN where a push produced none), ``complete`` (False: the slot was reset
    or imported over before the post-roll was full) and ``seq`` (the order in which the clips were opened)."""

    def __init__(self, slot, raised_at, first_hop, audio, scores, complete, seq):
        self.slot, self.raised_at, self.first_hop, self.seq = int(slot), int(raised_at), int(first_hop), int(seq)
        self.audio, self.scores, self.complete = audio, scores, bool(complete)

    @property
    def hops(self):
        return int(self.scores.size)

    def write_wav(self, path):
        """16 kHz mono 16-bit PCM (stdlib ``wave``); an fp32 clip goes through the pcm16 rule."""
        pcm = self.audio if self.audio.dtype == np.int16 else pcm16_reference(self.audio)
        with wave.open(path, "wb") as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(16000)
            w.writeframes(pcm.astype("<i2").tobytes())

    def __repr__(self):
        return (f"Clip(slot={self.slot}, raised_at={self.raised_at}, first_hop={self.first_hop}, hops={self.hops}, "
                f"complete={self.complete}, seq={self.seq}, {self.audio.dtype})")


def _clips_of(pool, audio, cscores, hop):
    """The finished entries of host copies of the pool -> ``Clip`` objects ordered by seq.  ``audio`` / ``cscores`` hold
    one row per finished entry, in the order of ``np.flatnonzero(finished)``."""
    done = np.flatnonzero((pool[:, 0] == COMPLETE) | (pool[:, 0] == TRUNCATED))
    out = []
    for row, e in enumerate(done):
        status, slot, raised_at, first_hop, hops, seq = (int(v) for v in pool[e])
        out.append(Clip(slot, raised_at, first_hop, audio[row, :hops * hop].copy(), cscores[row, :hops].copy(), status == COMPLETE, seq))
    return sorted(out, key=lambda c: c.seq)


class EvidencePolicy:
    """What is kept around an alarm; see the module docstring for the function.

    pre (None, or 0 to 65535): hops kept before the raising hop; None means ``window // hop - 1`` of the scorer it is put
    around.  post (0 to 65535): hops kept after the raising hop.  clips (1 to 8192): pool entries; an alarm raised while
    none is free is counted ``dropped``.  encoding: "fp32" stores the samples bit for bit, "pcm16" as int16."""

    def __init__(self, pre=None, post=8, clips=64, encoding="fp32"):
        self.pre = None if pre is None else integer("pre", pre, 0, MAX_HOPS)
        self.post = integer("post", post, 0, MAX_HOPS)
        self.clips = integer("clips", clips, 1, MAX_CLIPS)
        if not isinstance(encoding, str) or encoding not in ENCODINGS:
            raise ValueError(f"encoding {encoding!r}: one of {ENCODINGS}")
        self.encoding = encoding

    def params(self):
        """What identifies this policy (plain ints and strings; pre None = taken from the scorer's window)."""
        return dict(pre=self.pre, post=self.post, clips=self.clips, encoding=self.encoding)

    def pre_for(self, hop, window=None):
        """``pre`` for a scorer of this ``hop`` and ``window``; the ring and a clip stay below 2^31 samples."""
        hop = integer("hop", hop, 1, N_MAX)
        if self.pre is not None:
            pre = self.pre
        else:
            if window is None:
                raise ValueError("pre=None takes window // hop - 1: give the window")
            pre = integer("window // hop - 1", integer("window", window, 1, N_MAX) // hop - 1, 0, MAX_HOPS)
        if (pre + 1 + self.post) * hop > N_MAX:
            raise ValueError(f"a clip of {pre + 1 + self.post} hops of {hop} samples: below 2^31 samples")
        return pre

    # ---- the numpy restatement -------------------------------------------------------------------------------------------
    def new_state(self, S, hop, window=None):
        """Host mirrors of the device state of S new streams and an empty pool: a dict of numpy arrays ``hist``, ``sring``,
        ``rec``, ``left``, ``pool``, ``audio``, ``cscores``, ``counters`` (shapes and dtypes as in the module docstring)."""
        pre = self.pre_for(hop, window)
        P, L = pre + 1, pre + 1 + self.post
        return dict(hist=np.zeros((S, P * hop), np.float32), sring=np.zeros((S, P), np.float32), rec=np.full(S, -1, np.int32),
                    left=np.zeros(S, np.int32), pool=np.zeros((self.clips, 6), np.int32),
                    audio=np.zeros((self.clips, L * hop), np.float32 if self.encoding == "fp32" else np.int16),
                    cscores=np.zeros((self.clips, L), np.float32), counters=np.zeros(4, np.int32))

    def _encode(self, x):
        return x if self.encoding == "fp32" else pcm16_reference(x)

    def step_reference(self, state, hops, slots, hop_index, scores, verdict_state):
        """One update in numpy, row by row.  state: the mirrors of ``new_state``, UPDATED IN PLACE; hops (A, hop) float32;
        slots (A,) distinct ints (None: every slot); hop_index an int or (A,) ints >= 1; scores (A,) fp32 or None (all NaN);
        verdict_state (S, 4) ints, the verdict state rows after this push's verdict update."""
        hist, sring, rec, left, pool = (state[k] for k in ("hist", "sring", "rec", "left", "pool"))
        audio, cscores, counters = state["audio"], state["cscores"], state["counters"]
        S, P = sring.shape
        hop, pre, L = hist.shape[1] // P, P - 1, cscores.shape[1]
        if L != P + self.post or pool.shape != (self.clips, 6) or audio.shape != (self.clips, L * hop):
            raise ValueError("the state was not made by this policy's new_state")
        b = slots_of(slots, S)
        A = b.size
        x = np.asarray(hops)
        if x.dtype != np.float32 or x.shape != (A, hop):
            raise ValueError(f"hops: a float32 array of shape {(A, hop)}")
        k = np.broadcast_to(np.asarray(hop_index, dtype=np.int64).reshape(-1), (A,)) if np.ndim(hop_index) == 0 \
            else np.asarray(hop_index, dtype=np.int64).reshape(-1)
        s = np.full(A, np.nan, np.float32) if scores is None else np.asarray(scores, dtype=np.float32).reshape(-1)
        vst = np.asarray(verdict_state)
        if k.size != A or s.size != A or vst.shape != (S, 4):
            raise ValueError("slots, hops, hop_index and scores name the same rows; verdict_state is (S, 4)")
        if A and (k.min() < 1 or k.max() > N_MAX):
            raise ValueError("hop_index: 1 or more, below 2^31")
        free = [int(e) for e in np.flatnonzero(pool[:, 0] == FREE)]  # fixed during the update, taken in ascending index
        for i in range(A):
            slot, ki = int(b[i]), int(k[i])
            c = (ki - 1) % P
            hist[slot, c * hop:(c + 1) * hop] = x[i]
            sring[slot, c] = s[i]
            up = int(vst[slot, 2]) == 1 and int(vst[slot, 3]) == ki
            e = int(rec[slot])
            if e >= 0:
                counters[3] += up
                at = int(pool[e, 4])
                audio[e, at * hop:(at + 1) * hop] = self._encode(x[i])
                cscores[e, at] = s[i]
                pool[e, 4] = at + 1
                left[slot] -= 1
                if left[slot] == 0:
                    pool[e, 0] = COMPLETE
                    rec[slot] = -1
            elif up:
                counters[0] += 1
                if not free:
                    counters[2] += 1
                    continue
                e = free.pop(0)
                f = max(1, ki - pre)
                n = ki - f + 1
                pool[e] = (COMPLETE if self.post == 0 else RECORDING, slot, ki, f, n, counters[1])
                counters[1] += 1
                for j in range(n):
                    cc = (f - 1 + j) % P
                    audio[e, j * hop:(j + 1) * hop] = self._encode(hist[slot, cc * hop:(cc + 1) * hop])
                    cscores[e, j] = sring[slot, cc]
                if self.post > 0:
                    rec[slot], left[slot] = e, self.post
        return state

    @staticmethod
    def reset_reference(state, slots):
        """``Evidence.reset`` on the mirrors: a clip being recorded by a named slot is TRUNCATED, ``rec = -1``, ``left = 0``."""
        for slot in slots_of(slots, state["rec"].size):
            if state["rec"][slot] >= 0:
                state["pool"][state["rec"][slot], 0] = TRUNCATED
            state["rec"][slot], state["left"][slot] = -1, 0

    @staticmethod
    def take_reference(state):
        """``Evidence.take_clips`` on the mirrors -> the finished clips ordered by seq; their entries become FREE."""
        pool = state["pool"]
        done = np.flatnonzero((pool[:, 0] == COMPLETE) | (pool[:, 0] == TRUNCATED))
        hop = state["hist"].shape[1] // state["sring"].shape[1]
        out = _clips_of(pool, state["audio"][done], state["cscores"][done], hop)
        pool[done, 0] = FREE
        return out

    def run_reference(self, hops, scores, verdict_states, window=None):
        """S fresh streams over T hops each, ONE ROW PER UPDATE (hop t of slot 0, of slot 1, ...: the definition's own order).
        hops (T, S, hop) float32; scores (T, S) fp32, NaN where a hop produced no score; verdict_states (T, S, 4) ints, the
        verdict state rows after each hop.  -> the state mirrors after the last hop."""
        x = np.asarray(hops)
        T, S, hop = x.shape
        sc, vs = np.asarray(scores, dtype=np.float32).reshape(T, S), np.asarray(verdict_states).reshape(T, S, 4)
        state = self.new_state(S, hop, window)
        for t in range(T):
            for slot in range(S):
                self.step_reference(state, x[t, slot:slot + 1], [slot], t + 1, sc[t, slot:slot + 1], vs[t])
        return state


class Evidence(SlotTable):
    """The pre-roll rings of ``S`` slots and the clip pool under ``policy`` on ``device``, for hops of ``hop`` samples; see
    the module docstring.  ``update`` is one pinned upload of the header and two launches, with no synchronisation;
    ``take_clips()`` is the only read-back of the layer (``stats()`` reads the counters when asked).  window: needed only
    for a policy with ``pre=None``."""

    def __init__(self, S, policy, hop, device="cuda", window=None):
        S, self.policy = slot_count(S, policy, EvidencePolicy), policy
        self.pre = policy.pre_for(hop, window)
        self.hop, self.post, self.clips = int(hop), policy.post, policy.clips
        self.P, self.L = self.pre + 1, self.pre + 1 + self.post
        # the session state: the raw ring rows (a hop's position is a function of its hop number, so they move as they are;
        # ``reset`` leaves them: ``first_hop >= 1`` keeps a new session from reading them).  ``rec``, ``left``, the pool
        # and the counters belong to the scorer, not to a session
        self._allocate(S, device, Field("evidence_hist", "hist", (self.P * self.hop,), torch.float32),
                       Field("evidence_scores", "sring", (self.P,), torch.float32))
        dev = self.device
        self.rec = torch.full((self.S,), -1, dtype=torch.int32, device=dev)
        self.left = torch.zeros(self.S, dtype=torch.int32, device=dev)
        # (one header row more than the pool has entries: where ``reset`` sends the writes of slots that are not recording)
        self._pool = torch.zeros(self.clips + 1, 6, dtype=torch.int32, device=dev)
        self.audio = torch.zeros(self.clips, self.L * self.hop, dtype=torch.float32 if policy.encoding == "fp32" else torch.int16, device=dev)
        self.cscores = torch.zeros(self.clips, self.L, dtype=torch.float32, device=dev)
        self.counters = torch.zeros(4, dtype=torch.int32, device=dev)
        self._claim = torch.full((self.S,), N_MAX, dtype=torch.int32, device=dev)  # scratch of afx_k_evidence_mark
        self._work = torch.zeros(self.S, 4, dtype=torch.int32, device=dev)

    @property
    def pool(self):
        """(clips, 6) int32 on the device: the clip headers ``(status, slot, raised_at, first_hop, hops, seq)``."""
        return self._pool[:self.clips]

    # ---- the update ------------------------------------------------------------------------------------------------------
    def update(self, chunk, slots=None, *, hop_index, scores=None, verdict_state):
        """chunk: (A, hop) fp32 on the device, row i the hop of slot slots[i] (None: every slot, in order; the slots are
        distinct); hop_index: an int or (A,) ints on the host, 1 or more; scores: (A,) fp32 on the device (any stride) or
        None: every score is NaN; verdict_state: (S, 4) int32 on the device, ``Verdicts.st`` after this push's update.  One
        pinned upload, two launches, no synchronisation."""
        b = slots_of(slots, self.S)
        A = b.size
        if (not isinstance(chunk, torch.Tensor) or chunk.dtype != torch.float32 or chunk.shape != (A, self.hop)
                or chunk.device != self.device):
            raise ValueError(f"chunk: an fp32 tensor of shape {(A, self.hop)} on {self.device}")
        if scores is not None and (not isinstance(scores, torch.Tensor) or scores.dtype != torch.float32 or scores.shape != (A,)
                                   or scores.device != self.device):
            raise ValueError(f"scores: an fp32 tensor of shape {(A,)} on {self.device}, or None")
        if (not isinstance(verdict_state, torch.Tensor) or verdict_state.dtype != torch.int32 or verdict_state.shape != (self.S, 4)
                or verdict_state.device != self.device):
            raise ValueError(f"verdict_state: an int32 tensor of shape {(self.S, 4)} on {self.device}")
        k = hop_indices(hop_index, A, 1)
        if not A:
            return
        need_gpu(self.device, "evidence is recorded")
        if scores is not None and A > 1 and scores.stride(0) < 1:  # (an expanded view: the kernel reads scores[i * stride])
            scores = scores.contiguous()
        chunk, vst = chunk.contiguous(), verdict_state.contiguous()
        with torch.cuda.device(self.device):
            d = upload_pairs(b, k, self.device)
            check(call_on(self.hist, lib().afx_k_evidence_mark, ptr(d), A, ptr(vst), self.S, self.pre, self.post, ptr(self.rec),
                          ptr(self.left), ptr(self._claim), ptr(self._pool), self.clips, ptr(self.counters), ptr(self._work)))
            check(call_on(self.hist, lib().afx_k_evidence_copy, ptr(chunk), ptr(scores), 1 if scores is None else max(scores.stride(0), 1),
                          ptr(d), ptr(self._work), A, self.hop, self.pre, self.post, ptr(self.hist), ptr(self.sring), self.S,
                          ptr(self.audio), ptr(self.cscores), self.clips, ENCODINGS.index(self.policy.encoding)))

    # ---- sessions ------------------------------------------------------------------------------------------------------------
    def reset(self, slots):
        """The named slots begin a new stream: a clip one of them is recording becomes TRUNCATED (kept with the hops it
        has), ``rec = -1``, ``left = 0``.  The rings are left as they are.  No synchronisation."""
        b = slots_of(slots, self.S)
        if b.size:
            with _on(self.device):
                rows = torch.from_numpy(b).to(self.device)
                r = self.rec[rows].long()
                self._pool[:, 0].index_fill_(0, torch.where(r >= 0, r, torch.full_like(r, self.clips)), TRUNCATED)
                self._pool[self.clips, 0] = FREE
                self.rec[rows] = -1
                self.left[rows] = 0

    def import_rows(self, slots, *rows):
        """The named slots take the (checked) ring rows; what they were recording is TRUNCATED, as in ``reset``."""
        self.reset(slots)
        super().import_rows(slots, *rows)

    # ---- the read-back -------------------------------------------------------------------------------------------------------
    def _to_host(self, *tensors):
        """Host copies of device tensors (pinned, one synchronisation for all of them)."""
        if self.device.type != "cuda":
            return [t.clone() for t in tensors]
        out = []
        for t in tensors:
            host = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
            host.copy_(t, non_blocking=True)
            out.append(host)
        torch.cuda.current_stream(self.device).synchronize()
        return out

    def take_clips(self):
        """The clips finished since the last call (COMPLETE, or TRUNCATED by a reset), as ``Clip`` objects ordered by
        ``seq``; their pool entries become FREE.  The one read-back of this layer: the headers first, then only the finished
        clips' audio and scores (as far as the longest of them goes)."""
        with _on(self.device):
            pool = self._to_host(self.pool)[0].numpy()
            done = np.flatnonzero((pool[:, 0] == COMPLETE) | (pool[:, 0] == TRUNCATED))
            if not done.size:
                return []
            rows = torch.from_numpy(done).to(self.device)
            hops = int(pool[done, 4].max())
            audio = self.audio.index_select(0, rows)[:, :hops * self.hop].contiguous()
            cscores = self.cscores.index_select(0, rows)[:, :hops].contiguous()
            self._pool[:, 0].index_fill_(0, rows, FREE)
            audio, cscores = (t.numpy() for t in self._to_host(audio, cscores))
        return _clips_of(pool, audio, cscores, self.hop)

    def stats(self):
        """Host ints: ``raised`` (alarms raised on a slot that was not recording), ``recorded`` (clips opened), ``dropped``
        (raises that found no free entry), ``merged`` (raises while the slot was recording), and the pool's ``free``,
        ``recording`` and ``finished`` entries.  Reads the counters and the headers back."""
        with _on(self.device):
            c, status = self._to_host(self.counters, self.pool[:, 0].contiguous())
            c, status = c.tolist(), status.numpy()
        return dict(raised=c[0], recorded=c[1], dropped=c[2], merged=c[3], free=int((status == FREE).sum()),
                    recording=int((status == RECORDING).sum()), finished=int((status >= COMPLETE).sum()))


class EvidenceScorer(Layer):
    """``scorer`` (a ``VerdictScorer``: the one kind this layer goes around, ``afx._layer.EXACTLY``) with the evidence
    recorder behind it under ``policy``; see the module docstring.  It presents the surface the fronts and the gate drive an
    inner scorer through and goes where the verdict layer goes:
    ``JitterScorer(GatedScorer(EvidenceScorer(VerdictScorer(CascadeScorer(...), vpolicy), epolicy)), 8000, "mulaw", depth)``.

    ``push`` returns exactly what the inner ``push`` returns, then records the hops it was given: one small upload and two
    launches, no synchronisation.  A KV-cached ``None`` (no score yet) still stores the audio, with NaN scores.  ``alarm``,
    ``smoothed``, ``alarm_since`` and ``take_events()`` are the verdict layer's; ``take_clips()`` is the only read-back of
    this one, ``stats()`` its counters.

    Sessions: the part of a ``StreamState`` is ``evidence_hist`` ((n, (pre + 1) hop) fp32) and ``evidence_scores``
    ((n, pre + 1) fp32), the raw ring rows, meta ``evidence`` (format) and ``evidence_pre`` (``post``, ``clips`` and
    ``encoding`` may differ where the sessions go): a moved session keeps its pre-roll.  A recording in progress does NOT
    move: the clip stays in the source's pool, keeps filling while the source slot is pushed, and is TRUNCATED when the
    source slot is next reset or imported over, as is what the destination's named slots were recording.  The pool and the
    counters belong to the scorer, not to a session."""

    layer = "evidence"
    _part = "evidence part (it was not exported by an EvidenceScorer)"

    def __init__(self, scorer, policy):
        super().__init__(scorer)
        self.policy = policy
        self.evidence = self._own(Evidence(scorer.S, policy, scorer.hop, scorer.device, window=scorer.window))

    @property
    def alarm(self):
        return self.scorer.alarm

    @property
    def smoothed(self):
        return self.scorer.smoothed

    @property
    def alarm_since(self):
        return self.scorer.alarm_since

    def take_events(self):
        """``VerdictScorer.take_events``."""
        return self.scorer.take_events()

    def take_clips(self):
        """``Evidence.take_clips``: the finished clips ordered by seq; the only read-back of this layer."""
        return self.evidence.take_clips()

    def stats(self):
        """``Evidence.stats``."""
        return self.evidence.stats()

    def push(self, chunk, slots=None):
        """chunk and slots: the inner scorer's own rule -> exactly what the inner ``push`` returns; then one
        ``Evidence.update`` over the named slots with ``hop_index = samples_seen // hop``."""
        need_gpu(self.device, "hops are scored and recorded")
        inner = self.scorer
        scores = inner.push(chunk, slots)
        idx = self._named(slots)
        A = len(idx)
        if not A:
            return scores
        returned_scores(scores, A, self.device)
        self.evidence.update(chunk.to(self.device, torch.float32), idx, hop_index=(inner.samples_seen[idx] // self.hop).numpy(),
                             scores=scores, verdict_state=inner.verdicts.st)
        return scores

    # ---- sessions (afx._layer.Layer) -----------------------------------------------------------------------------------------
    def _meta(self):
        return dict(evidence=EVIDENCE_FORMAT, evidence_pre=self.evidence.pre)
