"""Provenance: the jitter buffer knows which samples it made up, and a stream's score is withheld while too much of the
model's window is such audio.

``afx.jitter`` writes audio that nobody spoke -- the last 10 ms or the last pitch period repeated, zeros, comfort noise --
into the window of a model whose job is to flag synthetic speech.  What that does to the false-alarm rate is not measured
(there is no corpus to measure it with); which samples are ours is known exactly.  This module carries a "made up here" mark,
one per 16 kHz sample, on the device from the jitter buffer through its pending ring and a speech gate's compaction to a
layer next to the quality layer: ``ProvenanceScorer(scorer, policy)`` hands on the inner score bit for bit, or the quiet NaN
("cannot judge", as ``afx.quality`` does for a clipped microphone: the verdict layer raises nothing on it, the evidence layer
records nothing).

The function (also stated in include/afx.h).

Marks.  E is a slot's played-out stream as ``afx.jitter`` defines it.  C[i] = 1 where released index i was not received: it
was loss-concealed in any mode, "zero" included, or is comfort noise; else C[i] = 0 (``oracle.jitter.RefSlot.kinds``: C[i] = 1
where ``kinds[i] != "r"``).

At 16 kHz.  Output sample K of the slot's resampled stream, counted from the session's origin, has the mark
c16[K] = C[floor(K * M / L)], L / M the slot's up / down ratio (the identity: c16 = C).  This is the newest input sample of
K's filter support, on purpose: a release that moves the playout counter from N to N + n_in produces exactly the outputs whose
source lies in [N, N + n_in), and a synthetic run [u, v) of that release is exactly the outputs [ceil(u L / M), ceil(v L / M)),
so the host needs no history.  The mark LEADS the filter's centre by the resampler's delay, 0.6 to 1.25 ms (``Resampler.delay``
16 kHz samples): a synthetic sample's energy is centred that much later than its mark.  That does not matter for a count over
a window of seconds.  ``marks16(kinds, L, M)`` is the statement in numpy.

Per frame, per hop.  n[f] is the sum of c16 over the 16 kHz frame f: ``gate.frame`` samples where a gate stands in the chain,
otherwise the whole hop.  A hop's count c is the sum of n over its frames.  Behind a gate the gated stream's frame counts are
the kept frames' counts, in order, exactly as the samples are compacted.

The layer.  ``ProvenancePolicy(max_share=0.05, abstain=True)``; ``W = ceil(window / hop)``, 1 <= W <= 1024;
``limit = int(floor(float64(fp32(max_share)) * W * hop))``.  Per slot the state is ``p_ring`` ((S, W) int32: the count of hop k
at (k - 1) mod W), ``p_state`` ((S, 2) int32 = (total, valid); (0, 1) for a new stream) and ``p_totals`` ((S, 3) int32: hops,
synthetic samples, hops that were not valid -- the scores withheld, or with ``abstain`` off the ones that would have been).
All counters saturate at 2^31 - 1.  An update names rows (slot (distinct), k >= 1, c in 0..hop, score)::

    p_ring[b, (k-1) mod W] = c
    total   = the sum of the ring entries of hops max(1, k-W+1)..k          (never before the session's first hop)
    valid   = total <= limit
    p_state[b] = (total, valid);  p_totals[b] += (1, c, 1 - valid)
    meas[i] = (c, total, valid), 3 int32
    out[i]  = the score, bit for bit, when valid or abstain is off, else the quiet NaN 0x7fc00000

A row with a slot outside [0, S), k < 1 or c outside 0..hop is skipped whole: the state is untouched, its ``meas`` row is -1
and its score passes.  ``reset`` makes ``p_state`` (0, 1) and clears ``p_totals`` only: the bound k >= 1 keeps a new session
from reading the ring entries of the one before it (the quality layer's rule, for the same reason).  It is all integer
arithmetic; the kernel (``afx_k_provenance``, one thread per row) equals ``ProvenancePolicy.step_reference`` exactly.

How the counts travel.  No ``push`` signature changes.  Directly before it pushes a round of hops, whatever stands above
calls ``note_synthetic(counts, slots)`` on the next object below that takes notes (``note_target``): counts are int32 on
the device.  The next ``push`` of exactly those slots consumes the note; any other ``push`` raises ValueError, and the note
is gone.  A ``push`` with no note counts 0 for every row: ``PacketScorer`` and ``ResamplingScorer`` make nothing up and note
nothing.  At construction a ``JitterScorer`` / ``MixedJitterScorer`` walks the ``.scorer`` links below it (``discover``); with
a provenance layer there it turns its lane on: a byte ring ``psyn`` (S, ring_len) parallel to its pending ring, one
("spans", rows) op per round directly after the round's release (rows of (slot, wpos, n, value) that partition every release
row's output range into received and synthetic runs; ``afx_k_prov_spans``) and at each pop one ``afx_k_prov_frames`` launch
that turns the popped hops of ``psyn`` into frame counts.  A ``GatedScorer`` with a plain ``SpeechGate`` or a ``ToneGate``
on the way is attached: it asks its gate launch for the mask, keeps a count ring ``gsyn`` (S, ring_len / frame) int32 parallel
to its sample ring (``afx_k_prov_compact`` after the gate launch, ``afx_k_prov_take`` at a pop) and notes the hop's sum to
whatever takes notes below it; its one read-back stays the only one.  A ``LookaheadGate`` (its mask is delayed) or a
``TurnScorer`` (its mask feeds turn buffers) on the way is refused under the policy's default ``through="plain"``.  With no
provenance layer below, nothing of the front or the gate changes in any respect.

Through pre-roll and turns (``ProvenancePolicy(through="all")``; ``through`` is an attribute of the policy, no part of
``params()`` and no part of a session).  Both layers move whole frames in a stated order, so the counts go the same way.

Behind a ``LookaheadGate`` the gated stream is the emitted frames in order (``keep'``), and its frame counts are n[g] over
the emitted g, in order: in numpy ``n[:decided][mask]`` with ``mask`` from ``LookaheadGate.gate_reference`` over the whole
stream, then sums of ``hop / frame``.  The attached gate owns ``gline`` ((S, pre) int32: the count of delayed frame g at block
g mod pre, parallel to ``line``; ``reset`` leaves it alone, nothing before a session's first frame is ever read) and its push
calls ``afx_k_prov_compact_la`` in the place of ``afx_k_prov_compact``, over the gate launch's own header and mask: the
count of an emitted frame comes out of ``gline`` where an earlier push brought the frame and out of the push's own counts
otherwise, and the push's last ``pre`` counts enter ``gline`` after every read.  ``afx_k_prov_take`` serves the pop unchanged.

Through a ``TurnScorer`` the turn recurrence copies kept frame j of a row to ``bufs[slot][open][n]``; ``bsyn`` ((S, 2,
max_frames) int32, parallel to ``bufs``) takes ``counts[j]`` at the same place (``afx_k_prov_turn``, launched directly before
``afx_k_turn`` with the same mask and header; it reads the turn state and never writes it).  The clip of a scored turn of m
frames is the turn tiled to ``max_frames`` frames, so its count is ``clip_count(n[first:end], max_frames)`` =
``np.resize(n[first:end], max_frames).sum()`` = ``q * sum(all m) + sum(the first rem)``, ``q, rem = divmod(max_frames, m)``
(``afx_k_prov_turn_sum``, beside ``afx_k_turn_collect`` over the same table): made-up audio is repeated with the turn.  That
count is noted to what takes notes below directly before the inner ``push``; the layer there stands around a scorer with
``hop == window``, so ``W = 1`` and ``limit = floor(share * window)``.  ``flush`` goes through the same tail; the close step
moves no frame and takes no note.  The limit of 512 frames per push holds for both chains.

Sessions: the layer's part of a ``StreamState`` is ``prov_ring`` ((n, W) int32), ``prov_state`` ((n, 2) int64) and
``prov_totals`` ((n, 3) int64), meta ``provenance`` (format) and ``provenance_window`` (W and hop); a front whose lane is on
adds ``jitter_syn`` (laid out as ``jitter_pending``, uint8), an attached gate ``gate_syn`` ((n, hop / frame) int64, -1 after
the fill).  Rows that cannot be a session's are refused: a count above ``frame`` or ``hop``, a total that is not the ring's
sum, a flag counted more often than hops.  A state without the front's or the gate's part imports with zeros; one with them
is refused by a chain without the layer.  The ring holds counts, so ``max_share`` and ``abstain`` may differ where a session
goes (``valid`` is set under the importing policy's limit, so a state whose new streams carry (0, 0) imports as well).  An
attached look-ahead gate adds ``gate_syn_line`` ((n, pre) int64: the delayed frames' counts, oldest first, zeros in front
where fewer than ``pre`` are delayed -- ``gate_line``'s layout; an entry outside 0..frame or a non-zero one in front of the
delayed frames is refused), an attached ``TurnScorer`` ``turn_syn`` ((n, max_frames) int64: the open turn's counts, then -1;
anything else after ``turn_frames`` or an entry outside 0..frame is refused; it lands in buffer 0 with ``turn_open``).  Both
follow ``gate_syn``'s rule: refused by an object that is not attached, and a state without them imports with zeros.

Out of scope: offline timelines and turns (no jitter buffer); counts or per-sample marks in evidence clips; a ``TurnScorer``
with pre-roll (not built); tuned thresholds (0.05 is an engineering default: there is no labelled corpus behind it); the
filter-delay offset of the mark.
"""
import numpy as np
import torch

from ._layer import N_MAX, Field, HopTable, WindowState, WithholdingLayer, fp32, hop_indices, need_gpu, slot_count, slots_of
from ._lib import call_on, check, lib, ptr
from .quality import MAX_HOP, QNAN_BITS, window_hops

PROVENANCE_FORMAT = 1  # layout of the provenance part of a StreamState: import_slots refuses any other
MAX_FRAMES = 512       # frames of a hop behind an attached gate (one afx_k_prov_compact workgroup)


def marks16(kinds, L, M):
    """c16 of a played-out stream: ``kinds`` (``oracle.jitter.RefSlot.kinds``, or any sequence that is "r" where the index
    was received) at the up / down ratio L / M -> (ceil(len * L / M),) uint8, c16[K] = C[floor(K * M / L)]."""
    C = np.fromiter((k != "r" for k in kinds), dtype=np.uint8, count=len(kinds))
    K = np.arange(-(-len(kinds) * L // M), dtype=np.int64)
    return C[K * M // L]


class ProvenanceState(WindowState):
    """Host mirrors of the whole provenance state of S slots: ``ring`` (S, W) int32, ``st`` (S, 2) int32 = (total, valid),
    ``totals`` (S, 3) int32; a new stream everywhere."""

    ring_dtype, new, n_totals = np.int32, (0, 1), 3


class ProvenancePolicy:
    """When a stream's score is withheld: while more than ``max_share`` (0..1, rounded to fp32 once) of the samples of the
    last ``W`` hops were made up by the jitter buffer.  abstain=False: count only, every score passes.  0.05 is an engineering
    default, not a tuned one."""

    def __init__(self, max_share=0.05, abstain=True, through="plain"):
        self.share32 = fp32("max_share", max_share, False)
        if self.share32 > 1:
            raise ValueError(f"max_share {max_share!r}: 0 to 1")
        if not isinstance(abstain, (bool, np.bool_)):
            raise ValueError(f"abstain: True or False, got {abstain!r}")
        if not isinstance(through, str) or through not in ("plain", "all"):
            raise ValueError(f'through: "plain" or "all", got {through!r}')
        self.max_share, self.abstain, self.through = float(self.share32), bool(abstain), through

    def params(self):
        """What identifies this policy (a float and a bool; ``through`` says which chains a front may build over the layer
        and is no part of a session)."""
        return dict(max_share=self.max_share, abstain=self.abstain)

    def limit(self, W, hop):
        """The synthetic samples a window of W hops of ``hop`` samples may hold: floor(float64(fp32(max_share)) * W * hop)."""
        return int(np.floor(np.float64(self.share32) * W * hop))

    # ---- the numpy restatement -------------------------------------------------------------------------------------------
    def step_reference(self, slots, counts, hop_index, scores, state, hop):
        """One update in numpy.  slots (A,) distinct ints, counts (A,) ints, hop_index an int or (A,) ints, scores (A,) fp32
        or None, hop the samples of a hop; ``state`` (a ``ProvenanceState`` of the whole scorer) is UPDATED IN PLACE -> ``(out,
        meas)``: (A,) float32 or None, and (A, 3) int32.  A row with ``hop_index < 1`` or a count outside 0..hop is skipped
        whole as the kernel skips it (its meas row is -1, its score passes)."""
        if not isinstance(state, ProvenanceState):
            raise ValueError("state: a ProvenanceState")
        S, W = state.ring.shape
        b = slots_of(slots, S)
        A = b.size
        c = np.asarray(counts)
        if c.dtype == bool or (c.size and not np.issubdtype(c.dtype, np.integer)) or c.ndim != 1 or c.size != A:
            raise ValueError("counts: one integer per named slot")
        c = c.astype(np.int64)
        if isinstance(hop, bool) or not isinstance(hop, (int, np.integer)) or not 1 <= hop <= MAX_HOP:
            raise ValueError(f"hop {hop!r}: 1 to {MAX_HOP}")
        k = hop_indices(hop_index, A).copy()
        s_in = None if scores is None else np.asarray(scores, dtype=np.float32).reshape(-1).copy()
        if s_in is not None and s_in.size != A:
            raise ValueError("slots, counts, hop_index and scores name the same rows")
        limit = self.limit(W, int(hop))
        meas = np.full((A, 3), -1, dtype=np.int32)
        out = None if s_in is None else s_in.copy()
        live = np.flatnonzero((k >= 1) & (c >= 0) & (c <= hop))
        if not live.size:
            return out, meas
        b, k, c = b[live], k[live], c[live]
        state.ring[b, (k - 1) % W] = c.astype(np.int32)
        i = np.arange(W, dtype=np.int64)[None, :]
        inside = i < np.minimum(k, W)[:, None]                  # hops k, k-1, ..: never before the session's first
        entries = state.ring[b[:, None], (k[:, None] - 1 - i) % W].astype(np.int64)
        total = (entries * inside).sum(axis=1)
        valid = total <= limit
        state.st[b] = np.stack([np.minimum(total, N_MAX), valid], axis=1).astype(np.int32)
        tot = state.totals[b].astype(np.int64)
        tot += np.stack([np.ones_like(c), c, 1 - valid.astype(np.int64)], axis=1)
        state.totals[b] = np.minimum(tot, N_MAX).astype(np.int32)
        meas[live] = np.stack([c, np.minimum(total, N_MAX), valid], axis=1).astype(np.int32)
        if out is not None and self.abstain:
            out.view(np.int32)[live[~valid]] = QNAN_BITS
        return out, meas

    def run_reference(self, counts, hop, window):
        """One fresh stream, hop by hop: counts (n,) ints, the synthetic samples of each hop -> ``(meas (n, 3) int32, valid
        (n,) bool)``: the measurement of every hop and whether the stream's score passes after it (a skipped hop passes)."""
        c = np.asarray(counts).reshape(-1)
        st = ProvenanceState(1, window_hops(window, hop))
        meas = np.zeros((c.size, 3), dtype=np.int32)
        for j in range(c.size):
            meas[j] = self.step_reference([0], c[j:j + 1], j + 1, None, st, hop)[1][0]
        return meas, meas[:, 2] != 0


class Provenance(HopTable):
    """The per-slot provenance state of ``S`` streams under ``policy`` for hops of ``hop`` samples and a window of ``window``
    samples, on ``device``; see the module docstring.  ``update`` is one pinned upload of the header and one
    ``afx_k_provenance`` launch, with no synchronisation; ``valid`` and ``synthetic`` are views of the state on the device;
    ``stats()`` is the only read-back."""

    meas_cols = 3

    def __init__(self, S, policy, hop, window, device="cuda"):
        S = slot_count(S, policy, ProvenancePolicy)
        self.W = window_hops(window, hop)
        self.policy, self.hop, self.window = policy, int(hop), int(window)
        self.limit = policy.limit(self.W, self.hop)
        # (``reset`` leaves the ring alone: a new session's window sum never reaches back before its first hop)
        self._allocate(S, device, Field("prov_ring", "ring", (self.W,), torch.int32),
                       Field("prov_state", "st", (2,), torch.int32, host=True, new=(0, 1)),
                       Field("prov_totals", "totals", (3,), torch.int32, host=True, new=0))

    @property
    def synthetic(self):
        """(S,) int32 on the device: the synthetic samples in each slot's window."""
        return self.st[:, 0]

    @property
    def valid(self):
        """(S,) bool on the device: which slots' scores pass (``total <= limit``; a new stream is valid)."""
        return self.st[:, 1] != 0

    def stats(self):
        """Per slot, since its last ``reset``: (S,) int64 host tensors ``hops``, ``synthetic`` (samples) and ``withheld`` (the
        hops that were not valid).  Reads ``p_totals`` back: the only read-back of this layer."""
        t = self.totals.to("cpu", torch.int64)
        return dict(hops=t[:, 0].clone(), synthetic=t[:, 1].clone(), withheld=t[:, 2].clone())

    def update(self, counts, slots=None, *, hop_index, scores=None):
        """counts: (A,) int32 on the device, row i the synthetic samples of the hop of slot slots[i] (None: every slot, in
        order; the slots are distinct); hop_index: an int or (A,) ints on the host, 1 or more; scores: (A,) fp32 on the device
        (any stride) or None -> ``(out, meas)`` on the device: (A,) fp32 or None, (A, 3) int32.  One pinned upload, one launch,
        no synchronisation."""
        b = slots_of(slots, self.S)
        A = b.size
        if (not isinstance(counts, torch.Tensor) or counts.dtype != torch.int32 or counts.shape != (A,)
                or counts.device != self.device):
            raise ValueError(f"counts: an int32 tensor of shape {(A,)} on {self.device}")
        k, scores = self._hop_rows(A, hop_index, scores)
        return self._update(counts.contiguous(), b, k, scores) if A else self._no_rows(scores)

    def _update(self, counts, slots, hop_index, scores):
        need_gpu(self.device, "hops are counted")
        with torch.cuda.device(self.device):
            d, meas, out = self._buffers(slots, hop_index, scores)
            check(call_on(self.ring, lib().afx_k_provenance, ptr(d), ptr(counts), ptr(scores),
                          1 if scores is None else max(scores.stride(0), 1), len(slots), self.hop, self.limit, int(self.policy.abstain),
                          ptr(self.ring), self.W, ptr(self.st), ptr(self.totals), self.S, ptr(meas), ptr(out)))
        return out, meas

    # ---- sessions ------------------------------------------------------------------------------------------------------------
    def check_rows(self, rows, n, seen):
        """Refuses (ValueError) what cannot be the state of n sessions of this window that have seen ``seen`` (n,) samples; ->
        (ring, st, totals), ``valid`` set under THIS policy's limit."""
        self.check_shapes(rows, n)
        ring, st, totals = rows[0], rows[1].cpu().clone(), rows[2].cpu()
        r = ring.cpu().to(torch.int64)
        if bool(((r < 0) | (r > self.hop)).any()):
            raise ValueError(f"import_slots: a hop counts more synthetic samples than its {self.hop} (or fewer than 0)")
        k = torch.as_tensor(seen, dtype=torch.int64).reshape(-1) // self.hop
        i = torch.arange(self.W)[None, :]
        inside = i < k.clamp(max=self.W)[:, None]
        total = (r.gather(1, (k[:, None] - 1 - i) % self.W) * inside).sum(dim=1)
        if bool((st[:, 0] != total.clamp(max=N_MAX)).any()):
            raise ValueError("import_slots: a session's synthetic total is not the sum of its window's ring entries")
        if bool(((st[:, 1] != 0) & (st[:, 1] != 1)).any()):
            raise ValueError("import_slots: a session's valid flag is 0 or 1")
        if bool(((totals < 0) | (totals > N_MAX)).any()) or bool((totals[:, 2] > totals[:, 0]).any()):
            raise ValueError("import_slots: a session's totals are negative, or hops were withheld more often than hops were seen")
        st[:, 1] = (total <= self.limit).to(torch.int64)
        return ring, st, totals


def note_target(scorer):
    """The next object at or below ``scorer`` (along the ``.scorer`` links) that takes notes, or None."""
    while scorer is not None and not callable(getattr(scorer, "note_synthetic", None)):
        scorer = getattr(scorer, "scorer", None)
    return scorer


def clip_count(frame_counts, max_frames):
    """The count of a scored turn's clip: ``frame_counts`` (m,) ints, the counts of the turn's m frames (1 <= m <=
    max_frames) -> the count of the turn tiled to ``max_frames`` frames, ``q * sum(all m) + sum(the first rem)`` with
    ``q, rem = divmod(max_frames, m)``: ``np.resize(frame_counts, max_frames).sum()``, as ``afx_k_prov_turn_sum`` computes it."""
    c = np.asarray(frame_counts).reshape(-1)
    if c.dtype == bool or (c.size and not np.issubdtype(c.dtype, np.integer)):
        raise ValueError("frame_counts: integers")
    if isinstance(max_frames, bool) or not isinstance(max_frames, (int, np.integer)) or not 1 <= c.size <= max_frames:
        raise ValueError(f"a turn of {c.size} frames: 1 to max_frames = {max_frames!r}")
    c = c.astype(np.int64)
    q, rem = divmod(int(max_frames), c.size)
    return int(q * c.sum() + c[:rem].sum())


def discover(front):
    """What a jitter front does at construction: walks the ``.scorer`` links below it; with no provenance layer there ->
    None and nothing changes.  With one: a ``GatedScorer`` with a plain ``SpeechGate`` or a ``ToneGate`` on the way is
    attached; a ``GatedScorer`` with a ``LookaheadGate`` or a ``TurnScorer`` on the way is attached where the layer's policy
    says ``through="all"`` and is a ValueError under ``through="plain"``, as is any other object of kind "gate" -> (the object
    the front notes its counts to, the samples of a frame of those counts, whether that object is an attached gate)."""
    from .turns import TurnScorer
    from .vad import GatedScorer, LookaheadGate
    chain, s = [], getattr(front, "scorer", None)
    while s is not None:
        chain.append(s)
        s = getattr(s, "scorer", None)
    layer = next((s for s in chain if getattr(s, "layer", None) == "provenance"), None)
    if layer is None:
        return None
    every = getattr(getattr(layer, "policy", None), "through", "plain") == "all"
    gated = None
    for s in chain:
        if getattr(s, "layer", None) == "provenance":
            break
        if getattr(s, "layer", None) == "gate":
            plain = isinstance(s, GatedScorer) and not isinstance(s.gate, LookaheadGate)
            if not plain and not (every and isinstance(s, (GatedScorer, TurnScorer))):
                what = "LookaheadGate (its mask is delayed)" if isinstance(s, GatedScorer) else f"{type(s).__name__} (its mask feeds turn buffers)"
                raise ValueError(f"a jitter front over a provenance layer: a {what} on the way is out of scope")
            if s.hop // s.gate.frame > MAX_FRAMES:
                raise ValueError(f"a jitter front over a provenance layer: a hop of at most {MAX_FRAMES} gate frames")
            gated = s
    if gated is not None:
        gated._attach_provenance()
        return gated, gated.gate.frame, True
    return note_target(front.scorer), front.scorer.hop, False


class ProvenanceScorer(WithholdingLayer):
    """``scorer`` (a streaming scorer, a cascade or a quality layer) with the provenance layer behind it under ``policy``;
    see the module docstring.  It goes where the quality layer goes, around it and inside the verdict layer:
    ``JitterScorer(GatedScorer(VerdictScorer(ProvenanceScorer(QualityScorer(inner, qpolicy), ppolicy), vpolicy)), 8000,
    "mulaw", depth)``.

    ``push`` runs the inner ``push``, then one update with the counts of the note it holds (``note_synthetic``; none: zeros)
    and ``hop_index = samples_seen // hop`` (one small upload, one launch, no synchronisation) and returns ``out``: the inner
    scores, bit for bit, with the quiet NaN where the slot is not valid (a KV-cached ``None`` stays ``None``; the hop is counted
    all the same).

    Results, all on the device: ``last_meas`` ((A, 3) int32 = (c, total, valid), the rows of the newest push), ``valid`` ((S,)
    bool), ``synthetic`` ((S,) int32, the window totals).  ``stats()`` is the only read-back.  Around a cascade ``verified``,
    ``verified_at`` and ``take_events`` are the cascade's, and with ``abstain`` on ``last_verified()`` has NaN for the
    verifier scores of the slots that are not valid."""

    layer = "provenance"
    _part = "provenance part (it was not exported by a ProvenanceScorer)"
    _does = "hops are scored and counted"

    def __init__(self, scorer, policy=None):
        super().__init__(scorer, ProvenancePolicy() if policy is None else policy, Provenance)
        self.provenance = self._table
        self._note = None  # (slots, counts) for the next push

    @property
    def synthetic(self):
        return self.provenance.synthetic

    def note_synthetic(self, counts, slots):
        """counts: (A,) int32 on the scorer's device, the synthetic samples of the hop the next ``push`` brings for each of
        ``slots`` (in its row order).  The next ``push`` must name exactly these slots; it consumes the note."""
        idx = self._named(slots)
        dev = self.provenance.device
        if not isinstance(counts, torch.Tensor) or counts.dtype != torch.int32 or counts.shape != (len(idx),) or counts.device != dev:
            raise ValueError(f"counts: an int32 tensor of shape {(len(idx),)} on {dev}")
        self._note = (idx, counts)

    def _operand(self, chunk, idx):
        """The counts of the note this push consumes, or zeros."""
        note, self._note = self._note, None
        if note is None:
            return torch.zeros(len(idx), dtype=torch.int32, device=self.provenance.device)
        if note[0] != idx:
            raise ValueError(f"the note names the slots {note[0]}, this push {idx}: a note is for the next push of exactly its slots")
        return note[1]

    # ---- sessions (afx._layer.Layer) -----------------------------------------------------------------------------------------
    def _meta(self):
        return dict(provenance=PROVENANCE_FORMAT, provenance_window=dict(W=self.provenance.W, hop=self.hop))
