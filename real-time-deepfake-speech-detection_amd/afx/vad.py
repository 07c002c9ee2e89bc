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

The contract of ``GatedScorer``: for a slot, let R be the concatenation of the hops it was pushed since its reset and G its
gated stream.  The slot's j-th non-NaN score equals, bit for bit, score j of a fresh inner scorer of the same kind pushed G
hop by hop, and it is emitted by the push in which sample ``(j + 1) * hop - 1`` of G was kept.  Nothing depends on the other
slots, on the order or subsets in which slots are named, or on session moves.  Behind a front, R is what that front's
contract defines it to be.

The one read-back.  Which slots advance depends on the audio, so a push copies ``kept`` (one int32 per named slot) to pinned
host memory and waits for it: A x 4 bytes once per hop.  Everything else (ring heads, fills, counters) is host arithmetic
on that number.
"""
import math

import numpy as np
import torch

from ._layer import Layer, StreamState, _on, check_pending, export_pending, import_pending, need_gpu, rows_on, upload_pairs
from ._lib import AfxError, call_on, check, lib, ptr

GATE_FORMAT = 1  # layout of the gate part of a StreamState: import_slots refuses any other
MAX_FRAMES = 512  # frames of a row one afx_k_gate launch takes (the library splits longer rows itself)


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
    def gate_reference(self, x, state=None):
        """The function in numpy.  x: host fp32 array of whole frames (1-D, a multiple of ``frame`` samples); state: what an
        earlier call returned (None: a new stream; it is not modified) -> (keep_mask (frames,) bool, the kept samples, the
        state after x).  Chunked at any frame boundaries with the state carried it gives what the whole stream gives."""
        x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
        if x.size % self.frame:
            raise ValueError(f"{x.size} samples are not whole frames of {self.frame}")
        st = self.new_state() if state is None else state
        nf, h = np.float32(st["nf"]), int(st["h"])
        E_floor, ratio, rise, nf_min, inf = self.E_floor, self.ratio32, self.rise32, self.nf_min, np.float32(np.inf)
        e_all = frame_energies(x, self.frame)
        keep = np.zeros(e_all.size, dtype=bool)
        with np.errstate(over="ignore"):
            for f, e in enumerate(e_all):
                fin = bool(e < inf)
                speech = fin and bool(e > max(E_floor, np.float32(ratio * nf)))
                if fin:
                    nf = max(nf_min, min(e, np.float32(nf * rise)))
                if speech:
                    h = self.hang
                keep[f] = speech or h > 0
                if not speech and h > 0:
                    h -= 1
        kept = x.reshape(-1, self.frame)[keep].reshape(-1).copy()
        return keep, kept, {"nf": np.float32(nf), "h": h}

    # ---- the device form ---------------------------------------------------------------------------------------------------
    def _launch(self, x, hdr, nf, h, ring, kept, mask=None):
        """afx_k_gate over the rows of x ((A, n) fp32 on the GPU, contiguous) with this gate's constants."""
        check(call_on(x, lib().afx_k_gate, ptr(x), x.shape[0], x.shape[1], ptr(hdr), self.frame, float(self.E_floor),
                      float(self.ratio32), float(self.rise32), self.hang, ptr(nf), ptr(h), ptr(ring), ring.shape[0], ring.shape[1],
                      ptr(kept), ptr(mask)))

    def gate(self, clips, return_mask=False):
        """The offline form: ``afx_k_gate`` over whole clips, each with fresh state.  clips: a list of 1-D CUDA fp32 tensors
        (any lengths) or a (B, n) CUDA tensor -> the list of kept-audio tensors (1-D, possibly empty), ready for
        ``model.forward_ragged``; with ``return_mask`` also the list of per-frame bool masks.  Trailing samples short of a
        whole frame are dropped.  One launch sequence and one read-back of the counts per distinct clip length."""
        clips = list(clips.unbind(0)) if isinstance(clips, torch.Tensor) and clips.ndim == 2 else list(clips)
        for c in clips:
            if not isinstance(c, torch.Tensor) or c.ndim != 1 or c.dtype != torch.float32:
                raise ValueError("gate: a list of 1-D fp32 tensors or a (B, n) tensor")
            if not c.is_cuda:
                raise AfxError("the gate runs on the GPU; there is no CPU fallback (gate_reference is the numpy restatement)")
        out, masks = [None] * len(clips), [None] * len(clips)
        groups = {}
        for i, c in enumerate(clips):
            groups.setdefault((c.device, c.numel() // self.frame), []).append(i)
        for (dev, frames), rows in groups.items():
            if frames == 0:
                for i in rows:
                    out[i] = torch.empty(0, dtype=torch.float32, device=dev)
                    masks[i] = torch.zeros(0, dtype=torch.bool, device=dev)
                continue
            n = frames * self.frame
            with torch.cuda.device(dev):
                for lo in range(0, len(rows), 65535):
                    part = rows[lo:lo + 65535]
                    A = len(part)
                    x = torch.stack([clips[i][:n] for i in part]).contiguous()
                    hdr = torch.stack([torch.arange(A, dtype=torch.int32), torch.zeros(A, dtype=torch.int32)], dim=1).to(dev)
                    nf = torch.full((A,), float("inf"), dtype=torch.float32, device=dev)
                    h = torch.zeros(A, dtype=torch.int32, device=dev)
                    ring = torch.empty(A, n, dtype=torch.float32, device=dev)
                    kept = torch.zeros(A, dtype=torch.int32, device=dev)
                    mask = torch.zeros(A, frames, dtype=torch.uint8, device=dev) if return_mask else None
                    self._launch(x, hdr, nf, h, ring, kept, mask)
                    for r, (i, k) in enumerate(zip(part, kept.tolist())):
                        out[i] = ring[r, :k].clone()
                        if return_mask:
                            masks[i] = mask[r].bool()
        return (out, masks) if return_mask else out


def emitted(scores):
    """``GatedScorer.push``'s result (or a FeedResult of a front around it) -> bool tensor: which entries are scores (a NaN
    stands for a push that completed no hop of speech)."""
    return ~torch.isnan(scores.scores if hasattr(scores, "scores") else scores)


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
    is the gate's ``samples_seen``.  Counters, a hangover or a noise floor that cannot be a gate's are refused."""

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
        if not A:
            return torch.empty(0, dtype=torch.float32, device=dev)
        slot = np.asarray(idx, dtype=np.int64)
        head, fill = self._head[slot], self._fill[slot]
        with torch.cuda.device(dev):
            hdr = upload_pairs(slot, (head + fill) % self.ring_len, dev)
            kept = torch.empty(A, dtype=torch.int32, device=dev)
            self.gate._launch(chunk.to(dev).contiguous(), hdr, self.nf, self.h, self.ring, kept)
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
                tab = torch.empty(3 * R, dtype=torch.int32, pin_memory=True)  # the pop table (slot, head), then the result rows
                tab.numpy()[:2 * R] = np.stack([slot[rows], head[rows]], axis=1).reshape(-1)
                tab.numpy()[2 * R:] = rows
                d = tab.to(dev, non_blocking=True)
                ready = torch.empty(R, hop, dtype=torch.float32, device=dev)
                check(call_on(self.ring, lib().afx_k_ingest_pop, ptr(self.ring), self.S, self.ring_len, ptr(d), R, hop, ptr(ready)))
                self._head[slot[rows]] = (head[rows] + hop) % self.ring_len
                self._fill[slot[rows]] = fill[rows] - hop
                sc = self.scorer.push(ready, slot[rows].tolist())
                if sc is None:
                    raise RuntimeError("the inner scorer emitted no score for a hop")
                if R == A:
                    out = sc.to(torch.float32)
                else:
                    out.index_copy_(0, d[2 * R:].long(), sc.to(torch.float32))
        return out

    def _reset(self, idx):
        """The noise floor (``nf = inf``), the hangover, the pending samples and the counters are dropped."""
        if idx:
            with _on(self.device):
                rows = rows_on(idx, self.device)
                self.nf[rows] = float("inf")
                self.h[rows] = 0
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
            return dict(gate_pending=export_pending(self.ring, idx, self._head[idx], self._fill[idx], self.hop),
                        gate_fill=torch.from_numpy(self._fill[idx]), gate_hang=self.h[rows].to("cpu", torch.int64),
                        gate_inner_seen=st.seen.clone(), gate_nf=self.nf[rows].clone())

    def _check(self, state, n):
        hop, t = self.hop, state.tensors
        counts = []
        for k in ("gate_fill", "gate_hang", "gate_inner_seen"):
            c = t[k].cpu().reshape(-1)
            if c.dtype != torch.int64 or c.numel() != n:
                raise ValueError(f"import_slots: {k} is (n,) int64")
            counts.append(c.numpy())
        fill, hang, inner_seen = counts
        seen = state.seen.numpy()
        pend, nf = t["gate_pending"], t["gate_nf"]
        check_pending("gate_pending", pend, fill, n, hop)
        if pend.shape[1] != hop:
            raise ValueError(f"import_slots: gate_pending {tuple(pend.shape)} is not {(n, hop)}")
        if tuple(nf.shape) != (n,) or nf.dtype != torch.float32:
            raise ValueError(f"import_slots: gate_nf {tuple(nf.shape)} {nf.dtype} is not {(n,)} float32")
        if ((fill >= hop) | (fill % self.gate.frame != 0)).any():
            raise ValueError(f"import_slots: a session's pending samples are not whole {self.gate.frame}-sample frames short of a hop")
        if ((inner_seen < 0) | (seen < 0) | (inner_seen % hop != 0) | (seen % hop != 0)).any():
            raise ValueError("import_slots: a session's sample count is not a whole number of hops")
        if (inner_seen + fill > seen).any():
            raise ValueError("import_slots: a session kept more samples than it was pushed")
        if ((hang < 0) | (hang > self.gate.hang)).any():
            raise ValueError(f"import_slots: a session's hangover is outside 0..{self.gate.hang} frames")
        nf_host = nf.cpu()
        if bool(torch.isnan(nf_host).any()) or bool((nf_host < float(self.gate.nf_min)).any()):
            raise ValueError(f"import_slots: a session's noise floor is NaN or below the gate's minimum {float(self.gate.nf_min)!r}")
        return pend, nf, hang, fill, seen

    def _import(self, idx, rows):
        pend, nf, hang, fill, seen = rows
        if idx:
            import_pending(self.ring, idx, pend)
            with _on(self.device):
                dev_rows = rows_on(idx, self.device)
                self.nf[dev_rows] = nf.to(self.device)
                self.h[dev_rows] = torch.from_numpy(hang).to(self.device, torch.int32)
            self._head[idx] = 0
            self._fill[idx] = fill
            self._seen[idx] = seen
