"""Packet front of the streaming scorers: bytes in, scores out.

A real-time service receives audio as encoded packets (G.711 mu-law / A-law or PCM, 10 - 60 ms each, a different size per
call, never aligned to the scorers' 250-ms hop), at the caller's sample rate.  ``PacketScorer`` wraps any of the three
streaming scorers and takes those packets as they arrive: ``feed(packets, slots)`` uploads the bytes of every packet in
one copy; on the GPU ``afx_k_ingest`` decodes them, resamples each slot's stream to 16 kHz at the phase the slot's stream
has reached and appends the result to the slot's pending ring; ``afx_k_ingest_pop`` hands every completed hop to the inner
scorer's non-paced ``push``.

The contract: let D be the decoded concatenation of everything a slot was fed since its reset and
R = ``Resampler(input_rate)(D)``, the offline kernel over the whole stream.  The slot's j-th score is, bit for bit, score
j of a fresh inner scorer pushed R hop by hop, and it is emitted by the ``feed`` / ``drain`` in which sample
(j+1)*hop - 1 of R became computable.  Nothing depends on where packets were cut, on the other slots, on the order slots
are named in, or on whether hops were scored at once or drained later.  It holds because (a) decoding is exact in fp32,
(b) output n of the causal polyphase filter reads inputs <= floor(n*M/L) whatever the chunking, and the ingest kernel gives
it the offline kernel's inputs, taps and fma order (the absolute counters N = samples received, n_done = ceil(N*L/M)
outputs made are kept here, on the host, and reduced to a phase p0 = n_done*M mod L and an offset
d0 = floor(n_done*M/L) - N >= 0 per packet), and (c) the inner scorers' non-paced push contract.

Nothing is read back from the device: how many outputs a packet completes is host arithmetic (``plan``), so ring
positions, phases and hop counts go up with the payload.  A ``feed`` is one host-to-device copy (payloads, each 16-byte
aligned, then the header / pop tables of every launch it will make) and a few launches; a ``drain`` uploads its pop tables.

Sessions: ``reset`` drops pending samples, filter history and counters with the inner session; ``export_slots`` adds
``ingest_pending`` ((n, max_pending*hop) fp32, left-aligned, zeros after), ``ingest_fill``, ``ingest_in`` ((n,) int64) and
``resample_hist`` to the inner ``StreamState``, with meta ``input_rate``, ``resampler`` and ``ingest``.  What is stored is
decoded: the encoding is no part of a state.
"""
import ctypes as C

import numpy as np
import torch

from ._lib import AfxError, call_on, check, lib, ptr
from .resample import FILTER_ID, Resampler
from .streaming import StreamState, _on

ENCODINGS = ("pcm_f32le", "pcm_s16le", "mulaw", "alaw")  # the library's encoding numbers 0..3
INGEST_FORMAT = 1  # layout of the ingest part of a StreamState: import_slots refuses any other
HDR = 8  # int32 per afx_k_ingest row: slot, byte offset, n_in, n_out, p0, d0, wpos, 0
ALIGN = 16  # every payload and table starts on a 16-byte boundary of the staging buffer
_SAMPLE = {"pcm_f32le": np.dtype("<f4"), "pcm_s16le": np.dtype("<i2"), "mulaw": np.dtype("u1"), "alaw": np.dtype("u1")}
_MAX_SAMPLES = 1 << 30
_ZEROS = bytes(ALIGN)
_STATE_KEYS = ("ingest_pending", "ingest_fill", "ingest_in", "resample_hist")
_META_KEYS = ("input_rate", "resampler", "ingest")


def _encoding(encoding):
    if encoding not in ENCODINGS:
        raise ValueError(f"encoding {encoding!r}: one of {ENCODINGS}")
    return encoding


def payload(packet, encoding):
    """One packet as a contiguous 1-D uint8 array of whole little-endian samples (no copy where the input allows it).
    ``packet``: bytes / bytearray / memoryview, or a 1-D numpy array / CPU tensor of uint8 or, for the PCM encodings, of the
    sample type.  Anything else, or bytes that split a sample, is a ValueError."""
    st = _SAMPLE[_encoding(encoding)]
    if isinstance(packet, torch.Tensor):
        if packet.is_cuda or packet.ndim != 1:
            raise ValueError("a packet tensor is 1-D and on the host")
        packet = packet.detach().contiguous().numpy()
    if isinstance(packet, (bytes, bytearray, memoryview)):
        a = np.frombuffer(packet, dtype=np.uint8)
    elif isinstance(packet, np.ndarray):
        if packet.ndim != 1:
            raise ValueError("a packet array is 1-D")
        if packet.dtype == np.uint8:
            a = np.ascontiguousarray(packet)
        elif st.itemsize > 1 and packet.dtype == st.newbyteorder("="):
            a = np.ascontiguousarray(packet, dtype=st).view(np.uint8)
        else:
            raise ValueError(f"a {encoding} packet array has dtype uint8" + (f" or {st.name}" if st.itemsize > 1 else "") +
                             f", got {packet.dtype}")
    else:
        raise ValueError(f"a packet is bytes, a bytearray, a memoryview, a numpy array or a CPU tensor, got {type(packet).__name__}")
    if a.size % st.itemsize:
        raise ValueError(f"a {encoding} packet of {a.size} bytes splits a {st.itemsize}-byte sample")
    if a.size // st.itemsize >= _MAX_SAMPLES:
        raise ValueError("a packet holds fewer than 2**30 samples")
    return a


def plan(N, n, L, M):
    """A slot that has received N input samples gets n more -> (n_out, p0, d0): the 16 kHz samples they complete,
    ceil((N + n)*L/M) - ceil(N*L/M); the phase p0 = n_done*M mod L of the first of them (n_done = ceil(N*L/M)) and the
    position d0 = floor(n_done*M/L) - N >= 0 of its newest input from the first new sample.  Exact integer arithmetic on the
    absolute counters; the reduced values fit 32 bits however long the session."""
    N, n = int(N), int(n)
    done = -(-N * L // M)
    return -(-(N + n) * L // M) - done, done * M % L, done * M // L - N


def layout(sizes):
    """Byte offsets of blocks of ``sizes`` bytes laid out back to back, each on an ALIGN boundary -> (offsets, total)."""
    ends = np.cumsum(-(-np.asarray(sizes, dtype=np.int64).reshape(-1) // ALIGN) * ALIGN)
    return [0] + ends[:-1].tolist() if ends.size else [], int(ends[-1]) if ends.size else 0


def pack(payloads, tables, pinned=False):
    """The staging buffer of a feed: the payloads (bytes or uint8 arrays), then the int tables of its launches, each block
    ALIGN-aligned -> (uint8 host tensor, payload offsets, table offsets).  pinned: page-locked memory (the upload is then
    one asynchronous copy)."""
    blocks = list(payloads) + [np.ascontiguousarray(t).reshape(-1).view(np.uint8) for t in tables]
    sizes = np.fromiter(map(len, blocks), dtype=np.int64, count=len(blocks))
    offs, total = layout(sizes)
    buf = torch.empty(total, dtype=torch.uint8, pin_memory=pinned)
    parts = blocks
    if (sizes % ALIGN).any():  # zeros up to the next boundary after every block that ends off one
        parts = []
        for b in blocks:
            parts.append(b)
            if len(b) % ALIGN:
                parts.append(_ZEROS[:-len(b) % ALIGN])
    buf.numpy()[:] = np.frombuffer(b"".join(parts), dtype=np.uint8)
    return buf, offs[:len(payloads)], offs[len(payloads):]


def _at(t, off):
    return C.c_void_p(t.data_ptr() + off)


def decode(data, encoding, device="cuda"):
    """One packet or a whole file of ``encoding`` -> (n,) fp32 on the GPU: the device decode ``PacketScorer`` runs
    (pcm_s16le v / 32768; G.711 to the 16-bit linear value, / 32768; exact)."""
    a = payload(data, encoding)
    n = a.size // _SAMPLE[encoding].itemsize
    dev = torch.device(device)
    if dev.type != "cuda":
        raise AfxError("decode runs on the GPU; there is no CPU fallback")
    out = torch.empty(1, n, dtype=torch.float32, device=dev)
    if n == 0:
        return out[0]
    hdr = np.array([[0, 0, n, n, 0, 0, 0, 0]], dtype=np.int32)
    buf, _, (th,) = pack([a], [hdr], pinned=True)
    with torch.cuda.device(dev):
        d = buf.to(dev, non_blocking=True)
        check(call_on(out, lib().afx_k_ingest, _at(d, 0), d.numel(), _at(d, th), 1, n, ENCODINGS.index(encoding), None, 1, 1, 1,
                      None, ptr(out), 1, n))
    return out[0]


class FeedResult:
    """What a ``feed`` / ``drain`` completed: ``counts`` (len(slots),) int64 on the host, the hops each named slot
    completed; ``scores`` (counts.sum(),) fp32 on the scorer's device, the first named slot's scores in hop order, then the
    second's, ...; ``split()``: the per-slot score tensors (views)."""

    def __init__(self, counts, scores):
        self.counts, self.scores = counts, scores

    def split(self):
        return list(self.scores.split(self.counts.tolist()))


class PacketScorer:
    """``scorer`` (a SlidingWindowScorer, IncrementalScorer or KVCachedScorer) fed encoded packets of any size at
    ``input_rate`` Hz (any integer 8 000 - 192 000) in ``encoding`` (``ENCODINGS``); see the module docstring for the
    contract.  ``max_pending``: the whole hops a slot may buffer between ``feed(..., score=False)`` and ``drain``."""

    def __init__(self, scorer, input_rate, encoding="pcm_f32le", max_pending=4):
        self.encoding = _encoding(encoding)
        if isinstance(max_pending, bool) or not isinstance(max_pending, int) or max_pending < 1:
            raise ValueError("max_pending: a positive number of hops")
        self.rs = Resampler(input_rate, scorer.device)  # (a bad rate is a ValueError here)
        self.scorer, self.input_rate, self.hop, self.max_pending = scorer, self.rs.rate, scorer.hop, max_pending
        self.L, self.M = self.rs.L, self.rs.M
        # one hop beyond max_pending: a scoring feed always finds room for a packet's next samples after it has popped the
        # whole hops (a slot then holds < hop samples, and one input sample makes at most ceil(L/M) = 2)
        self.ring_len = (max_pending + 1) * self.hop
        self.ring = torch.zeros(scorer.S, self.ring_len, dtype=torch.float32, device=scorer.device)
        self.hist = torch.zeros(scorer.S, self.rs.history, dtype=torch.float32, device=scorer.device)
        self._head = torch.zeros(scorer.S, dtype=torch.int64)  # ring position of each slot's oldest pending sample (host)
        self._fill = torch.zeros(scorer.S, dtype=torch.int64)  # pending samples per slot (host)
        self._in = torch.zeros(scorer.S, dtype=torch.int64)  # input-rate samples per slot since its reset (host)

    @property
    def S(self):
        return self.scorer.S

    @property
    def device(self):
        return self.scorer.device

    @property
    def delay(self):
        """The resampled stream's lag behind resample_poly's centred output, in 16 kHz samples."""
        return self.rs.delay

    @property
    def samples_seen(self):
        """(S,) int64: the 16 kHz samples each slot's inner session has been pushed since its last ``reset``."""
        return self.scorer.samples_seen

    @property
    def pending(self):
        """(S,) int64: the 16 kHz samples waiting in each slot's buffer."""
        return self._fill.clone()

    @property
    def samples_in(self):
        """(S,) int64: the input-rate samples each slot received since its last ``reset``."""
        return self._in.clone()

    # ---- planning (host arithmetic only) ---------------------------------------------------------------------------
    def _plan(self, idx, sizes, offs, score):
        """The launches of a feed / drain over the slots ``idx`` (sizes[i] new samples for idx[i], their payload at byte
        offs[i]; None: a drain) -> (ops, per-slot hop counts, the counters after it).  ops: ("ingest", header rows, the
        largest n_out) and ("pop", (A, 2) table of slot and ring head, the slots).  No state changes here.  int64 arrays over
        the named slots (distinct); the products stay below 2**63 for sessions of less than 2**48 samples."""
        head, fill, nin = self._head.numpy().copy(), self._fill.numpy().copy(), self._in.numpy().copy()
        L, M, R, hop, bps = self.L, self.M, self.ring_len, self.hop, _SAMPLE[self.encoding].itemsize
        slot = np.asarray(idx, dtype=np.int64).reshape(-1)
        size = np.zeros(len(idx), dtype=np.int64) if sizes is None else np.asarray(sizes, dtype=np.int64).reshape(-1)
        offs = np.zeros(len(idx), dtype=np.int64) if offs is None else np.asarray(offs, dtype=np.int64).reshape(-1)
        done = np.zeros(len(idx), dtype=np.int64)  # samples of each packet already planned
        counts = np.zeros(len(idx), dtype=np.int64)
        ops = []
        while True:
            left = np.flatnonzero(done < size)
            s = slot[left]
            made = -(-nin[s] * L // M)
            m = np.minimum(size[left] - done[left], (made + R - fill[s]) * M // L - nin[s])  # what the ring has room for
            left, s, made, m = left[m > 0], s[m > 0], made[m > 0], m[m > 0]
            if left.size:
                n_out = -(-(nin[s] + m) * L // M) - made
                rows = np.zeros((left.size, HDR), dtype=np.int32)
                for c, v in enumerate((s, offs[left] + done[left] * bps, m, n_out, made * M % L, made * M // L - nin[s],
                                       (head[s] + fill[s]) % R)):
                    rows[:, c] = v
                ops.append(("ingest", rows, int(n_out.max())))
                done[left] += m
                nin[s] += m
                fill[s] += n_out
            while score:
                ready = fill[slot] >= hop
                if not ready.any():
                    break
                s = slot[ready]
                ops.append(("pop", np.stack([s, head[s]], axis=1).astype(np.int32), s.tolist()))
                head[s] = (head[s] + hop) % R
                fill[s] -= hop
                counts += ready
            if not (done < size).any():
                break
            if not left.size and not score:
                raise ValueError("a slot's buffer is full")  # (feed validates this before planning: not reached)
        return ops, counts.tolist(), (head.tolist(), fill.tolist(), nin.tolist())

    def _packets(self, packets, idx):
        """-> (one block of whole samples per named slot: bytes as they are, anything else through ``payload``; their byte
        counts)."""
        if isinstance(packets, (bytes, bytearray, memoryview, np.ndarray, torch.Tensor)):
            raise ValueError("packets: a list with one packet per named slot")
        packets = list(packets)
        if len(packets) != len(idx):
            raise ValueError(f"{len(packets)} packets for {len(idx)} named slots")
        bps = _SAMPLE[self.encoding].itemsize
        out = [p if type(p) is bytes else payload(p, self.encoding) for p in packets]
        nbytes = np.fromiter(map(len, out), dtype=np.int64, count=len(out))
        for i in np.flatnonzero((nbytes % bps != 0) | (nbytes // bps >= _MAX_SAMPLES)):
            payload(out[i], self.encoding)  # (raises, with the message)
        return out, nbytes

    # ---- the public calls --------------------------------------------------------------------------------------------
    def feed(self, packets, slots, score=True):
        """packets[i]: the next bytes of slot slots[i]'s stream, any length (0 included).  score=True: every hop a named
        slot completes is scored (in rounds, while the packets are ingested; afterwards no named slot holds a whole hop).
        score=False: the packets are decoded, resampled and buffered only (``drain`` scores them); a slot whose buffer would
        hold more than ``max_pending`` hops is a ValueError.  Everything is checked before anything changes.  -> FeedResult."""
        idx = self.scorer._slot_list(slots, ordered=True)
        pay, nbytes = self._packets(packets, idx)
        sizes = nbytes // _SAMPLE[self.encoding].itemsize
        if not score and idx:
            N, n = self._in.numpy()[idx], sizes
            after = self._fill.numpy()[idx] - (-(N + n) * self.L // self.M) + (-N * self.L // self.M)  # fill + n_out
            over = np.flatnonzero(after > self.max_pending * self.hop)
            if over.size:
                raise ValueError(f"slot {idx[over[0]]} would hold {after[over[0]]} pending samples, more than max_pending = "
                                 f"{self.max_pending} hops of {self.hop}: drain it first")
        offs, total = layout(nbytes)
        if total >= 1 << 31:
            raise ValueError("a feed carries less than 2 GiB")
        return self._run(idx, pay, sizes, offs, score)

    def drain(self, slots=None):
        """Score every completed hop of the named (default: all) slots -> FeedResult."""
        idx = list(range(self.S)) if slots is None else self.scorer._slot_list(slots, ordered=True)
        return self._run(idx, [], None, None, True)

    def _run(self, idx, pay, sizes, offs, score):
        ops, counts, (head, fill, nin) = self._plan(idx, sizes, offs, score)
        dev = self.device
        counts = torch.tensor(counts, dtype=torch.int64)
        if not ops:
            return FeedResult(counts, torch.empty(0, dtype=torch.float32, device=dev))
        if dev.type != "cuda":
            raise AfxError("packets are decoded, resampled and scored on the GPU; there is no CPU fallback")
        # where each score of the result sits in the concatenation of the pop rounds' outputs (a table when it is not in order)
        pos, base = {s: [] for s in idx}, 0
        for op in ops:
            if op[0] == "pop":
                for k, s in enumerate(op[2]):
                    pos[s].append(base + k)
                base += len(op[2])
        perm = [p for s in idx for p in pos[s]]
        tables = [op[1] for op in ops]
        if perm != list(range(base)):
            tables.append(np.array(perm, dtype=np.int64))
        buf, _, toffs = pack(pay, tables, pinned=True)
        enc, taps = ENCODINGS.index(self.encoding), (None if self.rs.identity else ptr(self.rs.taps))
        T = 1 if self.rs.identity else self.rs.T
        outs = []
        with torch.cuda.device(dev):
            d = buf.to(dev, non_blocking=True)  # the one upload
            for op, off in zip(ops, toffs):
                if op[0] == "ingest":
                    check(call_on(self.ring, lib().afx_k_ingest, _at(d, 0), d.numel(), _at(d, off), len(op[1]), int(op[2]), enc,
                                  taps, self.L, self.M, T, ptr(self.hist) if T > 1 else None, ptr(self.ring), self.S,
                                  self.ring_len))
                else:
                    chunk = torch.empty(len(op[2]), self.hop, dtype=torch.float32, device=dev)
                    check(call_on(self.ring, lib().afx_k_ingest_pop, ptr(self.ring), self.S, self.ring_len, _at(d, off),
                                  len(op[2]), self.hop, ptr(chunk)))
                    sc = self.scorer.push(chunk, op[2])
                    if sc is None:
                        raise RuntimeError("the inner scorer emitted no score for a hop")
                    outs.append(sc)
            # (the counters follow the device state: set once every launch of the plan has been issued)
            self._head, self._fill, self._in = (torch.tensor(v, dtype=torch.int64) for v in (head, fill, nin))
            scores = torch.cat(outs) if outs else torch.empty(0, dtype=torch.float32, device=dev)
            if len(tables) > len(ops):
                scores = scores.index_select(0, d[toffs[-1]:toffs[-1] + 8 * base].view(torch.int64))
        return FeedResult(counts, scores)

    # ---- sessions ----------------------------------------------------------------------------------------------------
    def reset(self, slots):
        """The named slots begin a new stream: inner session, pending samples, filter history and counters are dropped."""
        idx = self.scorer._slot_list(slots)
        self.scorer.reset(idx)
        if idx:
            self._head[idx] = 0
            self._fill[idx] = 0
            self._in[idx] = 0
            if self.hist.shape[1]:
                self.hist[idx] = 0.0

    def state_meta(self):
        return dict(self.scorer.state_meta(), input_rate=self.input_rate, resampler=FILTER_ID, ingest=INGEST_FORMAT)

    def export_slots(self, slots):
        """The inner scorer's ``StreamState`` of the named slots plus their pending samples (decoded, at 16 kHz), counters
        and filter history.  No byte of the scorer changes."""
        idx = self.scorer._slot_list(slots, ordered=True)
        st = self.scorer.export_slots(idx)
        dev = self.device
        with _on(dev):
            rows = torch.tensor(idx, dtype=torch.long, device=dev)
            fill = self._fill[idx]
            j = torch.arange(self.max_pending * self.hop)
            cols = (self._head[idx][:, None] + j) % self.ring_len
            pend = self.ring[rows[:, None], cols.to(dev)]
            pend.masked_fill_((j[None, :] >= fill[:, None]).to(dev), 0.0)
            tensors = dict(st.tensors, ingest_pending=pend, ingest_fill=fill.clone(), ingest_in=self._in[idx].clone(),
                           resample_hist=self.hist.index_select(0, rows))
        return StreamState(dict(st.meta, input_rate=self.input_rate, resampler=FILTER_ID, ingest=INGEST_FORMAT), st.seen, tensors)

    def import_slots(self, slots, state):
        """The named slots take over the sessions of ``state``, a state of a PacketScorer at the same input rate, filter and
        ingest format whose pending samples fit this scorer's ``max_pending``; anything else is a ValueError before
        anything changes."""
        idx = self.scorer._slot_list(slots, ordered=True)
        if not isinstance(state, StreamState):
            raise ValueError("import_slots takes a StreamState (export_slots / StreamState.from_state_dict)")
        if any(k not in state.tensors for k in _STATE_KEYS) or any(k not in state.meta for k in _META_KEYS):
            raise ValueError("import_slots: the state has no packet-ingest part (it was not exported by a PacketScorer)")
        mine = dict(input_rate=self.input_rate, resampler=FILTER_ID, ingest=INGEST_FORMAT)
        for k in _META_KEYS:
            if state.meta[k] != mine[k]:
                raise ValueError(f"import_slots: the state's {k} {state.meta[k]!r} is not this scorer's {mine[k]!r}")
        n = len(state)
        pend, h = state.tensors["ingest_pending"], state.tensors["resample_hist"]
        fill, nin = state.tensors["ingest_fill"].cpu().reshape(-1), state.tensors["ingest_in"].cpu().reshape(-1)
        if fill.dtype != torch.int64 or nin.dtype != torch.int64 or fill.numel() != n or nin.numel() != n:
            raise ValueError("import_slots: ingest_fill / ingest_in are (n,) int64")
        if pend.ndim != 2 or pend.shape[0] != n or pend.dtype != torch.float32:
            raise ValueError(f"import_slots: ingest_pending {tuple(pend.shape)} {pend.dtype} is not (n, pending) float32")
        if tuple(h.shape) != (n, self.rs.history) or h.dtype != torch.float32:
            raise ValueError(f"import_slots: resample_hist {tuple(h.shape)} {h.dtype} does not fit this scorer "
                             f"({(n, self.rs.history)} float32)")
        if bool((fill < 0).any()) or bool((fill > pend.shape[1]).any()) or bool((fill > self.max_pending * self.hop).any()):
            raise ValueError(f"import_slots: a session holds more pending samples than max_pending = {self.max_pending} hops "
                             f"of {self.hop} (or than its own buffer)")
        made = torch.tensor([-(-int(v) * self.L // self.M) for v in nin.tolist()], dtype=torch.int64)
        if bool((nin < 0).any()) or not torch.equal(made, state.seen + fill):
            raise ValueError("import_slots: a session's input count does not match its scored and pending samples")
        inner = StreamState({k: v for k, v in state.meta.items() if k not in _META_KEYS}, state.seen,
                            {k: t for k, t in state.tensors.items() if k not in _STATE_KEYS})
        self.scorer.import_slots(idx, inner)  # (refuses a foreign state before changing anything)
        if idx:
            dev = self.device
            with _on(dev):
                rows = torch.tensor(idx, dtype=torch.long, device=dev)
                w = min(pend.shape[1], self.ring_len)
                self.ring[rows, :w] = pend[:, :w].to(dev)
                if self.hist.shape[1]:
                    self.hist[rows] = h.to(dev)
            self._head[idx] = 0
            self._fill[idx] = fill
            self._in[idx] = nin
