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

from ._layer import check_pending, export_pending, import_pending, peel, rows_on, wrap
from ._lib import AfxError, call_on, check, lib, ptr
from .resample import FILTER_ID
from .streaming import FeedResult, _Front  # noqa: F401  (FeedResult is part of this module's interface)

ENCODINGS = ("pcm_f32le", "pcm_s16le", "mulaw", "alaw")  # the library's encoding numbers 0..3
INGEST_FORMAT = 1  # layout of the ingest part of a StreamState: import_slots refuses any other
HDR = 8  # int32 per afx_k_ingest row: slot, byte offset, n_in, n_out, p0, d0, wpos, 0
ALIGN = 16  # every payload and table starts on a 16-byte boundary of the staging buffer
_SAMPLE = {"pcm_f32le": np.dtype("<f4"), "pcm_s16le": np.dtype("<i2"), "mulaw": np.dtype("u1"), "alaw": np.dtype("u1")}
_MAX_SAMPLES = 1 << 30
_ZEROS = bytes(ALIGN)
_STATE_KEYS = ("ingest_pending", "ingest_fill", "ingest_in", "resample_hist")


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


class PacketScorer(_Front):
    """``scorer`` (a SlidingWindowScorer, IncrementalScorer or KVCachedScorer) fed encoded packets of any size at
    ``input_rate`` Hz (any integer 8 000 - 192 000) in ``encoding`` (``ENCODINGS``); see the module docstring for the
    contract.  ``max_pending``: the whole hops a slot may buffer between ``feed(..., score=False)`` and ``drain``."""

    _WORK = "decoded, resampled"

    def __init__(self, scorer, input_rate, encoding="pcm_f32le", max_pending=4):
        self.encoding = _encoding(encoding)
        if isinstance(max_pending, bool) or not isinstance(max_pending, int) or max_pending < 1:
            raise ValueError("max_pending: a positive number of hops")
        super().__init__(scorer, input_rate)
        self.L, self.M = self.rs.L, self.rs.M
        self._new_ring(max_pending)
        self.hist = torch.zeros(scorer.S, self.rs.history, dtype=torch.float32, device=scorer.device)
        self._head = np.zeros(scorer.S, dtype=np.int64)  # ring position of each slot's oldest pending sample (host)
        self._fill = np.zeros(scorer.S, dtype=np.int64)  # pending samples per slot (host)
        self._in = np.zeros(scorer.S, dtype=np.int64)  # input-rate samples per slot since its reset (host)

    @property
    def samples_in(self):
        """(S,) int64: the input-rate samples each slot received since its last ``reset``."""
        return torch.from_numpy(self._in.copy())

    # ---- planning (host arithmetic only) ---------------------------------------------------------------------------
    def _plan(self, idx, sizes, offs, score):
        """The launches of a feed / drain over the slots ``idx`` (sizes[i] new samples for idx[i], their payload at byte
        offs[i]; None: a drain) -> (ops, per-slot hop counts, the counters after it).  ops: ("ingest", header rows, the
        largest n_out) and ("pop", (A, 2) table of slot and ring head, the slots).  No state changes here.  int64 arrays over
        the named slots (distinct); the products stay below 2**63 for sessions of less than 2**48 samples."""
        L, M, R, bps = self.L, self.M, self.ring_len, _SAMPLE[self.encoding].itemsize
        slot = np.asarray(idx, dtype=np.int64).reshape(-1)
        head, fill, nin = self._head[slot], self._fill[slot], self._in[slot]  # (copies: over the named slots from here on)
        size = np.zeros(len(idx), dtype=np.int64) if sizes is None else np.asarray(sizes, dtype=np.int64).reshape(-1)
        offs = np.zeros(len(idx), dtype=np.int64) if offs is None else np.asarray(offs, dtype=np.int64).reshape(-1)
        done = np.zeros(len(idx), dtype=np.int64)  # samples of each packet already planned
        counts = np.zeros(len(idx), dtype=np.int64)
        ops = []
        while True:
            k = np.flatnonzero(done < size)
            made = -(-nin[k] * L // M)
            m = np.minimum(size[k] - done[k], (made + R - fill[k]) * M // L - nin[k])  # what the ring has room for
            k, made, m = k[m > 0], made[m > 0], m[m > 0]
            if k.size:
                n_out = -(-(nin[k] + m) * L // M) - made
                rows = np.zeros((k.size, HDR), dtype=np.int32)
                for c, v in enumerate((slot[k], offs[k] + done[k] * bps, m, n_out, made * M % L, made * M // L - nin[k],
                                       (head[k] + fill[k]) % R)):
                    rows[:, c] = v
                ops.append(("ingest", rows, int(n_out.max())))
                done[k] += m
                nin[k] += m
                fill[k] += n_out
            if score:
                self._pop_rounds(ops, slot, head, fill, counts)
            if not (done < size).any():
                break
            if not k.size and not score:
                raise ValueError("a slot's buffer is full")  # (feed validates this before planning: not reached)
        def of_all(mine, named):
            mine = mine.copy()
            mine[slot] = named
            return mine.tolist()

        return ops, counts.tolist(), (of_all(self._head, head), of_all(self._fill, fill), of_all(self._in, nin))

    # ---- the public calls --------------------------------------------------------------------------------------------
    def feed(self, packets, slots, score=True):
        """packets[i]: the next bytes of slot slots[i]'s stream, any length (0 included).  score=True: every hop a named
        slot completes is scored (in rounds, while the packets are ingested; afterwards no named slot holds a whole hop).
        score=False: the packets are decoded, resampled and buffered only (``drain`` scores them); a slot whose buffer would
        hold more than ``max_pending`` hops is a ValueError.  Everything is checked before anything changes.  -> FeedResult."""
        idx = self.scorer._slot_list(slots, ordered=True)
        pay, nbytes = self._packets(packets, len(idx), self.encoding)
        sizes = nbytes // _SAMPLE[self.encoding].itemsize
        if not score and idx:
            N, n = self._in[idx], sizes
            after = self._fill[idx] - (-(N + n) * self.L // self.M) + (-N * self.L // self.M)  # fill + n_out
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
        ops, counts, after = self._plan(idx, sizes, offs, score)
        enc, (taps, L, M, T) = ENCODINGS.index(self.encoding), self._filter()

        def ingest(d, off, op):
            check(call_on(self.ring, lib().afx_k_ingest, _at(d, 0), d.numel(), _at(d, off), len(op[1]), int(op[2]), enc, taps, L, M,
                          T, ptr(self.hist) if T > 1 else None, ptr(self.ring), self.S, self.ring_len))

        def commit():
            self._head, self._fill, self._in = (np.array(v, dtype=np.int64) for v in after)

        return self._execute(ops, idx, counts, pay, {"ingest": ingest}, commit)

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

    def _meta(self):
        return dict(input_rate=self.input_rate, resampler=FILTER_ID, ingest=INGEST_FORMAT)

    def export_slots(self, slots):
        """The inner scorer's ``StreamState`` of the named slots plus their pending samples (decoded, at 16 kHz), counters
        and filter history.  No byte of the scorer changes."""
        idx = self.scorer._slot_list(slots, ordered=True)
        st = self.scorer.export_slots(idx)
        return wrap(st, self._meta(), ingest_pending=export_pending(self.ring, idx, self._head[idx], self._fill[idx], self.max_pending * self.hop),
                    ingest_fill=torch.from_numpy(self._fill[idx]), ingest_in=torch.from_numpy(self._in[idx]),
                    resample_hist=self.hist.index_select(0, rows_on(idx, self.device)))

    def import_slots(self, slots, state):
        """The named slots take over the sessions of ``state``, a state of a PacketScorer at the same input rate, filter and
        ingest format whose pending samples fit this scorer's ``max_pending``; anything else is a ValueError before
        anything changes."""
        idx = self.scorer._slot_list(slots, ordered=True)
        inner = peel(state, _STATE_KEYS, self._meta(), "packet-ingest part (it was not exported by a PacketScorer)")
        n = len(state)
        pend, h = state.tensors["ingest_pending"], state.tensors["resample_hist"]
        fill, nin = state.tensors["ingest_fill"].cpu().reshape(-1), state.tensors["ingest_in"].cpu().reshape(-1)
        if fill.dtype != torch.int64 or nin.dtype != torch.int64 or fill.numel() != n or nin.numel() != n:
            raise ValueError("import_slots: ingest_fill / ingest_in are (n,) int64")
        fill, nin = fill.numpy(), nin.numpy()
        self._check_hist(h, n)
        check_pending("ingest_pending", pend, fill, n, self.max_pending * self.hop)
        made = np.array([-(-v * self.L // self.M) for v in nin.tolist()], dtype=np.int64)
        if (nin < 0).any() or not np.array_equal(made, state.seen.numpy() + fill):
            raise ValueError("import_slots: a session's input count does not match its scored and pending samples")
        self.scorer.import_slots(idx, inner)  # (refuses a foreign state before changing anything)
        if idx:
            import_pending(self.ring, idx, pend)
            if self.hist.shape[1]:
                self.hist[rows_on(idx, self.device)] = h.to(self.device)
            self._head[idx] = 0
            self._fill[idx] = fill
            self._in[idx] = nin
