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

Several formats on one scorer: ``MixedPacketScorer(scorer, formats)`` gives every slot its own (input_rate, encoding) out of
up to 16, chosen at ``reset``.  The contract: let (r, e) be slot s's format.  Slot s's scores are, bit for bit, those of
``PacketScorer(inner, r, e)`` fed the same packets -- the inner scorer's scores on ``Resampler(r)(decode(stream, e))`` --
whatever formats the other slots have, however the packets were cut and in whatever order slots are named.  It holds
because the format is a per-row value of the same launch (``afx_k_ingest_mixed``: the row's header names its format, the
workgroup runs the one-format kernel's validation, decoder and tile body with that format's filter) and the host plans each
row with its slot's own L, M and sample size.  A feed is still one upload, and one ingest launch plus one history launch
per round whatever the number of formats; the slot pool and the inner scorer's batch are shared by all of them.  A mixed
state carries the per-session ``ingest_rate`` ((n,) int64) in place of the meta's one ``input_rate``, ``resample_hist`` is
(n, Hs) with Hs the widest T - 1 of the scorer's formats (zeros beyond a session's own), and the meta says ``ingest_mixed``.

Expanded codecs: wherever a front takes an ``encoding`` it takes a name from ``ENCODINGS + CODECS`` (``afx.codecs``: ``dvi4``,
RFC 3551's IMA ADPCM, and the network-order ``pcm_s16be``, ``pcm_s24be`` and ``pcm_u8``, RTP's L16 / L24 / L8).  The kernels
of the fronts read a payload by random access, which a recurrence within a packet does not allow; so right after payload
validation a packet in a codec becomes, for every planner, a virtual pcm_f32le block of n = ``codecs.samples(nbytes, codec)``
samples in a *decoded zone* that follows the uploaded payloads and tables in the call's device buffer, each block 16-byte
aligned; a sub-range that starts k samples into the packet is read at zone offset + 4 k.  ``plan``, ``_plan``, the rounds and
all bookkeeping then run as they always did, on encoding 0 with 4 bytes per sample, behind one ("expand", rows, largest n) op
that is issued before the first ingest / place of the call (``afx_k_payload_expand``: one wave per DVI4 block, a map for the
PCM codecs).  The upload is still one pinned copy, into the front of a buffer that also holds the zone, and "a feed carries
less than 2 GiB" counts the zone.  A call without a packet in a codec plans and issues exactly what it did.  The contract is
the one above with D the concatenation of the decoded packets, ``codecs.reference`` of each: for DVI4 a packet is a block,
decoded from its own header whatever came before it; for the PCM codecs "however cut" holds on whole samples.  A DVI4 packet
under 4 bytes or with a header index above 88, and an s16be / s24be packet that splits a sample, are a ValueError before
anything changes.  States store decoded samples: a session exported from a ``dvi4`` scorer imports into a ``pcm_s16le`` one at
the same rate, and back.  A format of a ``MixedPacketScorer`` in a codec has a device entry that says encoding 0.  Out of
scope: stereo / channel de-interleave, G.722 / G.726 and other codecs whose state runs across packets, IMA file blocks (first
sample in the header), DVI4 encoding on the device.
"""
import ctypes as C

import numpy as np
import torch

from . import codecs
from ._layer import check_pending, export_pending, import_pending, peel, rows_on, wrap
from ._lib import AfxError, IngestFormat, call_on, check, lib, ptr
from .codecs import CODECS, EXPAND_HDR
from .resample import FILTER_ID, Resampler
from .streaming import FeedResult, _Front  # noqa: F401  (FeedResult is part of this module's interface)

ENCODINGS = ("pcm_f32le", "pcm_s16le", "mulaw", "alaw")  # the library's encoding numbers 0..3
INGEST_FORMAT = 1  # layout of the ingest part of a StreamState: import_slots refuses any other
HDR = 8  # int32 per afx_k_ingest row: slot, byte offset, n_in, n_out, p0, d0, wpos, 0 (afx_k_ingest_mixed: the format index)
MAX_FORMATS = 16  # formats of one MixedPacketScorer (the table afx_k_ingest_mixed takes by value)
ALIGN = 16  # every payload and table starts on a 16-byte boundary of the staging buffer
_SAMPLE = {"pcm_f32le": np.dtype("<f4"), "pcm_s16le": np.dtype("<i2"), "mulaw": np.dtype("u1"), "alaw": np.dtype("u1")}
_UNIT = dict({e: t.itemsize for e, t in _SAMPLE.items()}, **codecs.UNIT)  # bytes a packet is a whole number of
_MAX_SAMPLES = 1 << 30
_ZEROS = bytes(ALIGN)
_STATE_KEYS = ("ingest_pending", "ingest_fill", "ingest_in", "resample_hist")


def _encoding(encoding):
    if encoding not in ENCODINGS + CODECS:
        raise ValueError(f"encoding {encoding!r}: one of {ENCODINGS + CODECS}")
    return encoding


def device_encoding(encoding):
    """(the library's encoding number, bytes per sample) the ingest / place kernels read a packet of ``encoding`` with: its
    own for ``ENCODINGS``; an expanded codec's samples are read from the decoded zone, as pcm_f32le."""
    return (ENCODINGS.index(encoding), _SAMPLE[encoding].itemsize) if encoding in ENCODINGS else (0, 4)


def expand_zone(nbytes, offs, total, codec):
    """The decoded zone of a call whose packets (``nbytes`` bytes at the byte offsets ``offs`` of ``total`` payload bytes)
    are in the codecs ``codec`` (int64 array: the number in ``CODECS``, -1 for a packet the kernels read as it is) ->
    (samples per packet (for the others nothing is said: 0), the offset each packet is read at, the ``afx_k_payload_expand``
    rows or None, the zone's bytes).  A packet in a codec becomes a pcm_f32le block, 16-byte aligned, in a zone that is
    planned from byte ``total`` on: ``_Front._stage`` moves it behind the tables once their sizes are known."""
    nbytes, offs = np.asarray(nbytes, dtype=np.int64).reshape(-1), np.asarray(offs, dtype=np.int64).reshape(-1)
    e = np.flatnonzero(codec >= 0)
    n, at = np.zeros(len(nbytes), dtype=np.int64), offs.copy()
    if not e.size:
        return n, at, None, 0
    n[e] = codecs.samples_each(nbytes[e], codec[e])
    zoffs, zbytes = layout(4 * n[e])
    at[e] = total + np.asarray(zoffs, dtype=np.int64)
    e = e[n[e] > 0]
    rows = np.stack([offs[e], nbytes[e], at[e], codec[e]], axis=1).astype(np.int32) if e.size else None
    return n, at, rows, zbytes


def with_expand(ops, rows, kinds=("ingest", "place")):
    """``ops`` with one ("expand", rows, largest n) op before its first ingest / place op (none: ``ops`` as it is)."""
    first = next((i for i, op in enumerate(ops) if op[0] in kinds), None)
    if rows is None or first is None:
        return ops
    most = int(codecs.samples_each(rows[:, 1], rows[:, 3]).max())
    return ops[:first] + [("expand", rows, most)] + ops[first:]


def payload(packet, encoding):
    """One packet as a contiguous 1-D uint8 array of whole little-endian samples (no copy where the input allows it).
    ``packet``: bytes / bytearray / memoryview, or a 1-D numpy array / CPU tensor of uint8 or, for the PCM encodings, of the
    sample type.  Anything else, or bytes that split a sample, is a ValueError."""
    name = _encoding(encoding)
    st, unit = _SAMPLE.get(name, np.dtype("u1")), _UNIT[name]  # (a packet in a codec is bytes)
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
    if a.size % unit:
        raise ValueError(f"a {encoding} packet of {a.size} bytes splits a {unit}-byte sample")
    if name == "dvi4":
        codecs.dvi4_header(a)  # (a malformed block raises)
    if a.size // unit >= _MAX_SAMPLES:
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
    (pcm_s16le v / 32768; G.711 to the 16-bit linear value, / 32768; a codec of ``afx.codecs`` as stated there -- for dvi4
    ``data`` is one block; exact)."""
    a = payload(data, encoding)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise AfxError("decode runs on the GPU; there is no CPU fallback")
    if encoding in CODECS:  # one expand row: the payload, then its table, then the samples
        n = codecs.samples(a.size, encoding)
        if n == 0:
            return torch.empty(0, dtype=torch.float32, device=dev)
        (_, th), up = layout([a.size, 4 * EXPAND_HDR])
        buf, _, _ = pack([a], [np.array([[0, a.size, up, CODECS.index(encoding)]], dtype=np.int32)], pinned=True)
        with torch.cuda.device(dev):
            d = torch.empty(up + 4 * n, dtype=torch.uint8, device=dev)
            d[:up].copy_(buf, non_blocking=True)
            check(call_on(d, lib().afx_k_payload_expand, _at(d, 0), d.numel(), _at(d, th), 1, n))
        return d[up:].view(torch.float32)
    n = a.size // _SAMPLE[encoding].itemsize
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
    ``input_rate`` Hz (any integer 8 000 - 192 000) in ``encoding`` (``ENCODINGS`` or ``CODECS``); see the module docstring for the
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
    def _ratios(self, slot):
        """(L, M, bytes per sample, format index) of the slots ``slot``: int64 arrays over them."""
        n = len(slot)
        return (np.full(n, self.L, dtype=np.int64), np.full(n, self.M, dtype=np.int64),
                np.full(n, device_encoding(self.encoding)[1], dtype=np.int64), np.zeros(n, dtype=np.int64))

    def _payloads(self, packets, idx):
        """-> (one block per named slot, their byte counts, their sample counts as far as the kernels read them as they are,
        each packet's number in ``CODECS`` or -1), each packet read in its slot's encoding."""
        pay, nbytes = self._packets(packets, len(idx), self.encoding)
        c = CODECS.index(self.encoding) if self.encoding in CODECS else -1
        return pay, nbytes, nbytes // _UNIT[self.encoding], np.full(len(idx), c, dtype=np.int64)

    def _plan(self, idx, sizes, offs, score):
        """The launches of a feed / drain over the slots ``idx`` (sizes[i] new samples for idx[i], their payload at byte
        offs[i]; None: a drain) -> (ops, per-slot hop counts, the counters after it).  ops: ("ingest", header rows, the
        largest n_out) and ("pop", (A, 2) table of slot and ring head, the slots).  No state changes here.  int64 arrays over
        the named slots (distinct); the products stay below 2**63 for sessions of less than 2**48 samples."""
        R = self.ring_len
        slot = np.asarray(idx, dtype=np.int64).reshape(-1)
        L, M, bps, fmt = self._ratios(slot)
        head, fill, nin = self._head[slot], self._fill[slot], self._in[slot]  # (copies: over the named slots from here on)
        size = np.zeros(len(idx), dtype=np.int64) if sizes is None else np.asarray(sizes, dtype=np.int64).reshape(-1)
        offs = np.zeros(len(idx), dtype=np.int64) if offs is None else np.asarray(offs, dtype=np.int64).reshape(-1)
        done = np.zeros(len(idx), dtype=np.int64)  # samples of each packet already planned
        counts = np.zeros(len(idx), dtype=np.int64)
        ops = []
        while True:
            k = np.flatnonzero(done < size)
            made = -(-nin[k] * L[k] // M[k])
            m = np.minimum(size[k] - done[k], (made + R - fill[k]) * M[k] // L[k] - nin[k])  # what the ring has room for
            k, made, m = k[m > 0], made[m > 0], m[m > 0]
            if k.size:
                Lk, Mk = L[k], M[k]
                n_out = -(-(nin[k] + m) * Lk // Mk) - made
                rows = np.zeros((k.size, HDR), dtype=np.int32)
                for c, v in enumerate((slot[k], offs[k] + done[k] * bps[k], m, n_out, made * Mk % Lk, made * Mk // Lk - nin[k],
                                       (head[k] + fill[k]) % R, fmt[k])):
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
        return self._run(*self._plan_feed(packets, slots, score))

    def _plan_feed(self, packets, slots, score=True):
        """The checks and the plan of a ``feed`` -> what ``_run`` takes: (named slots, payload blocks, (ops, per-slot hop
        counts, the counters after it)).  No state changes.  Packets in a codec are planned as pcm_f32le blocks of the decoded
        zone (``expand_zone``), behind one "expand" op."""
        idx = self.scorer._slot_list(slots, ordered=True)
        pay, nbytes, sizes, codec = self._payloads(packets, idx)
        offs, total = layout(nbytes)
        n, offs, rows, zone = expand_zone(nbytes, offs, total, codec)
        sizes = np.where(codec >= 0, n, sizes)
        if not score and idx:
            N, n = self._in[idx], sizes
            L, M, _, _ = self._ratios(np.asarray(idx, dtype=np.int64))
            after = self._fill[idx] - (-(N + n) * L // M) + (-N * L // M)  # fill + n_out
            over = np.flatnonzero(after > self.max_pending * self.hop)
            if over.size:
                raise ValueError(f"slot {idx[over[0]]} would hold {after[over[0]]} pending samples, more than max_pending = "
                                 f"{self.max_pending} hops of {self.hop}: drain it first")
        if total + zone >= 1 << 31:
            raise ValueError("a feed carries less than 2 GiB")
        ops, counts, after = self._plan(idx, sizes, offs, score)
        return idx, pay, (with_expand(ops, rows), counts, after)

    def drain(self, slots=None):
        """Score every completed hop of the named (default: all) slots -> FeedResult."""
        idx = list(range(self.S)) if slots is None else self.scorer._slot_list(slots, ordered=True)
        return self._run(idx, [], self._plan(idx, None, None, True))

    def _ingest(self):
        """-> ingest(d, off, op): the launch of one ("ingest", rows, largest n_out) op whose table sits at byte ``off`` of the
        uploaded buffer ``d``."""
        enc, (taps, L, M, T) = device_encoding(self.encoding)[0], self._filter()

        def ingest(d, off, op):
            check(call_on(self.ring, lib().afx_k_ingest, _at(d, 0), d.numel(), _at(d, off), len(op[1]), int(op[2]), enc, taps, L, M,
                          T, ptr(self.hist) if T > 1 else None, ptr(self.ring), self.S, self.ring_len))

        return ingest

    def _run(self, idx, pay, planned):
        ops, counts, after = planned
        ingest = self._ingest()

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


def _format(f):
    """One (input_rate, encoding) pair, checked -> (rate as an int, encoding)."""
    from .resample import _rate
    if isinstance(f, (str, bytes)) or not hasattr(f, "__len__") or len(f) != 2:
        raise ValueError(f"a format is an (input_rate, encoding) pair, got {f!r}")
    return _rate(f[0]), _encoding(f[1])


class MixedPacketScorer(PacketScorer):
    """``scorer`` fed encoded packets, every slot in its own format out of ``formats``: 1 to 16 distinct
    (input_rate, encoding) pairs (rates as for ``Resampler``, encodings ``ENCODINGS`` or ``CODECS``); see the module docstring for the
    contract.  A slot's format is chosen at ``reset`` (a fresh scorer has every slot at format 0) and never changes between
    resets.  ``feed``, ``drain``, ``samples_in``, ``pending`` and ``samples_seen`` are ``PacketScorer``'s."""

    def __init__(self, scorer, formats, max_pending=4):
        if isinstance(formats, (str, bytes)) or not hasattr(formats, "__len__") or not hasattr(formats, "__iter__"):
            raise ValueError("formats: a sequence of (input_rate, encoding) pairs")
        fm = tuple(_format(f) for f in formats)
        if not 1 <= len(fm) <= MAX_FORMATS:
            raise ValueError(f"{len(fm)} formats: 1 to {MAX_FORMATS}")
        if len(set(fm)) != len(fm):
            raise ValueError("formats: a format is listed twice")
        if isinstance(max_pending, bool) or not isinstance(max_pending, int) or max_pending < 1:
            raise ValueError("max_pending: a positive number of hops")
        self.scorer, self.formats = scorer, fm
        self._rs = {}  # one Resampler per rate, shared by the formats at that rate
        for r, _ in fm:
            if r not in self._rs:
                self._rs[r] = Resampler(r, scorer.device)
        rs = [self._rs[r] for r, _ in fm]
        arr = lambda v: np.array(v, dtype=np.int64)
        # (a format in a codec reads its expanded samples: its device entry says encoding 0, 4 bytes per sample)
        self._frate, self._fenc = arr([r for r, _ in fm]), arr([device_encoding(e)[0] for _, e in fm])
        self._fL, self._fM = arr([x.L for x in rs]), arr([x.M for x in rs])
        self._fH = arr([0 if x.identity else x.T - 1 for x in rs])  # carried samples per format
        self._fbps = arr([device_encoding(e)[1] for _, e in fm])
        self._funit = arr([_UNIT[e] for _, e in fm])  # bytes a packet of the format is a whole number of
        self._fcodec = arr([CODECS.index(e) if e in CODECS else -1 for _, e in fm])
        self._fdelay = np.array([x.delay for x in rs], dtype=np.float64)
        self._fname = np.array([e for _, e in fm], dtype=object)
        self.Hs = int(self._fH.max())
        self._table = (IngestFormat * len(fm))()  # afx_k_ingest_mixed's host table (the taps are the Resamplers' tensors)
        for t, x, e in zip(self._table, rs, self._fenc.tolist()):
            t.taps = None if x.identity else x.taps.data_ptr()
            t.encoding, t.L, t.M, t.T = e, x.L, x.M, 1 if x.identity else x.T
        self._new_ring(max_pending)
        self.hist = torch.zeros(scorer.S, self.Hs, dtype=torch.float32, device=scorer.device)
        self._head = np.zeros(scorer.S, dtype=np.int64)
        self._fill = np.zeros(scorer.S, dtype=np.int64)
        self._in = np.zeros(scorer.S, dtype=np.int64)
        self._fmt = np.zeros(scorer.S, dtype=np.int64)  # format index of each slot (host)

    # ---- per-slot formats ------------------------------------------------------------------------------------------------
    @property
    def format_of(self):
        """(S,) int64: the index into ``formats`` of each slot's format."""
        return torch.from_numpy(self._fmt.copy())

    @property
    def rates(self):
        """(S,) int64: each slot's input rate in Hz."""
        return torch.from_numpy(self._frate[self._fmt])

    @property
    def delays(self):
        """(S,) float64: each slot's ``Resampler.delay``, the lag of its resampled stream in 16 kHz samples."""
        return torch.from_numpy(self._fdelay[self._fmt])

    @property
    def delay(self):
        raise AttributeError("a MixedPacketScorer has one delay per slot: delays")

    def _index(self, f):
        """A format given as an index into ``formats`` or as a pair -> its index."""
        if isinstance(f, (int, np.integer)) and not isinstance(f, bool):
            if not 0 <= f < len(self.formats):
                raise ValueError(f"format index {f} outside 0..{len(self.formats) - 1}")
            return int(f)
        f = _format(f)
        if f not in self.formats:
            raise ValueError(f"format {f!r} is not one of this scorer's {self.formats}")
        return self.formats.index(f)

    def _indices(self, formats, n):
        """``formats``: one format (index or pair) for n slots, or n of them -> (n,) int64 array of indices."""
        def one(f):
            return (isinstance(f, (int, np.integer)) and not isinstance(f, bool)) or (
                isinstance(f, (tuple, list)) and len(f) == 2 and isinstance(f[1], str))
        if isinstance(formats, torch.Tensor):
            formats = formats.tolist()
        if isinstance(formats, np.ndarray):
            formats = formats.tolist()
        if one(formats):
            return np.full(n, self._index(formats), dtype=np.int64)
        if isinstance(formats, (str, bytes)) or not hasattr(formats, "__len__"):
            raise ValueError("formats: one format (an index or an (input_rate, encoding) pair) or one per named slot")
        if len(formats) != n:
            raise ValueError(f"{len(formats)} formats for {n} named slots")
        return np.array([self._index(f) for f in formats], dtype=np.int64).reshape(n)

    def _ratios(self, slot):
        f = self._fmt[slot]
        return self._fL[f], self._fM[f], self._fbps[f], f

    def _payloads(self, packets, idx):
        f = self._fmt[np.asarray(idx, dtype=np.int64)]
        pay, nbytes = self._packets_each(packets, self._fname[f].tolist(), self._funit[f])
        return pay, nbytes, nbytes // self._funit[f], self._fcodec[f]

    def _ingest(self):
        nf, hist = len(self.formats), ptr(self.hist) if self.Hs else None

        def ingest(d, off, op):
            rows = op[1]
            most = np.zeros(nf, dtype=np.int32)  # per format the largest n_out of this launch
            for f in np.unique(rows[:, 7]).tolist():
                most[f] = rows[rows[:, 7] == f, 3].max()
            check(call_on(self.ring, lib().afx_k_ingest_mixed, _at(d, 0), d.numel(), _at(d, off), len(rows),
                          C.cast(self._table, C.c_void_p), nf, most.ctypes.data_as(C.c_void_p), hist, self.Hs, ptr(self.ring),
                          self.S, self.ring_len))

        return ingest

    # ---- sessions ----------------------------------------------------------------------------------------------------
    def reset(self, slots, formats=None):
        """The named slots begin a new stream in ``formats``: one format (an index into ``formats`` or a pair) for all of
        them, or one per named slot; None keeps each slot's format.  Everything is checked before anything changes."""
        idx = self.scorer._slot_list(slots, ordered=True)
        new = None if formats is None else self._indices(formats, len(idx))
        super().reset(idx)
        if idx and new is not None:
            self._fmt[idx] = new

    def _meta(self):
        return dict(resampler=FILTER_ID, ingest=INGEST_FORMAT, ingest_mixed=1)

    def export_slots(self, slots):
        """``PacketScorer.export_slots`` with the per-session ``ingest_rate`` ((n,) int64) and ``resample_hist`` (n, Hs),
        zeros beyond each session's own T - 1 (module docstring).  No byte of the scorer changes."""
        idx = self.scorer._slot_list(slots, ordered=True)
        st = super().export_slots(idx)
        return wrap(st, {}, ingest_rate=torch.from_numpy(self._frate[self._fmt[idx]]))

    def import_slots(self, slots, state, formats=None):
        """The named slots take over the sessions of ``state``: a state of a MixedPacketScorer, or of a plain
        ``PacketScorer`` (one ``input_rate`` in its meta), with the same filter and ingest format.  ``formats``: the format
        each session continues in (one for all or one per session, at the session's rate); default: this scorer's first
        format at the session's rate.  A rate this scorer does not list, a format at another rate than the session's, a
        history with non-zero columns beyond a session's own T - 1, pending samples beyond ``max_pending`` or counters that
        contradict each other are a ValueError before anything changes."""
        idx = self.scorer._slot_list(slots, ordered=True)
        what = "packet-ingest part (it was not exported by a PacketScorer or a MixedPacketScorer)"
        n = len(state) if hasattr(state, "seen") else 0
        if hasattr(state, "meta") and "ingest_mixed" not in state.meta and "input_rate" in state.meta:  # a plain PacketScorer's
            rate = state.meta["input_rate"]
            inner = peel(state, _STATE_KEYS, dict(input_rate=rate, resampler=FILTER_ID, ingest=INGEST_FORMAT), what)
            rates = np.full(n, rate, dtype=np.int64)
        else:
            inner = peel(state, _STATE_KEYS + ("ingest_rate",), self._meta(), what)
            rates = state.tensors["ingest_rate"].cpu().reshape(-1)
            if rates.dtype != torch.int64 or rates.numel() != n:
                raise ValueError("import_slots: ingest_rate is (n,) int64")
            rates = rates.numpy()
        if len(idx) != n:
            raise ValueError(f"the state holds {n} sessions for {len(idx)} named slots")
        if formats is None:
            first = {}
            for i, (r, _) in enumerate(self.formats):
                first.setdefault(r, i)
            missing = [r for r in rates.tolist() if r not in first]
            if missing:
                raise ValueError(f"import_slots: a session at {missing[0]} Hz, which is none of this scorer's rates {sorted(first)}")
            fmt = np.array([first[r] for r in rates.tolist()], dtype=np.int64)
        else:
            fmt = self._indices(formats, n)
            bad = np.flatnonzero(self._frate[fmt] != rates)
            if bad.size:
                raise ValueError(f"import_slots: session {bad[0]} is at {rates[bad[0]]} Hz, format {self.formats[fmt[bad[0]]]!r} is not")
        pend, h = state.tensors["ingest_pending"], state.tensors["resample_hist"]
        fill, nin = state.tensors["ingest_fill"].cpu().reshape(-1), state.tensors["ingest_in"].cpu().reshape(-1)
        if fill.dtype != torch.int64 or nin.dtype != torch.int64 or fill.numel() != n or nin.numel() != n:
            raise ValueError("import_slots: ingest_fill / ingest_in are (n,) int64")
        fill, nin = fill.numpy(), nin.numpy()
        own = self._fH[fmt]  # each session's own T - 1
        if h.ndim != 2 or h.shape[0] != n or h.dtype != torch.float32 or (n and h.shape[1] < own.max()):
            raise ValueError(f"import_slots: resample_hist {tuple(h.shape)} {h.dtype} does not hold its sessions' carried samples "
                             f"((n, >= {int(own.max()) if n else 0}) float32)")
        if n and h.shape[1] and bool((h.cpu() * (torch.arange(h.shape[1])[None, :] >= torch.from_numpy(own)[:, None])).ne(0).any()):
            raise ValueError("import_slots: resample_hist has non-zero columns beyond a session's own T - 1")
        check_pending("ingest_pending", pend, fill, n, self.max_pending * self.hop)
        made = np.array([-(-v * l // m) for v, l, m in zip(nin.tolist(), self._fL[fmt].tolist(), self._fM[fmt].tolist())], dtype=np.int64)
        if (nin < 0).any() or not np.array_equal(made, state.seen.numpy() + fill):
            raise ValueError("import_slots: a session's input count does not match its scored and pending samples")
        self.scorer.import_slots(idx, inner)  # (refuses a foreign state before changing anything)
        if idx:
            import_pending(self.ring, idx, pend)
            if self.Hs:
                w = min(self.Hs, h.shape[1])
                rows = rows_on(idx, self.device)
                self.hist[rows] = 0.0
                self.hist[rows, :w] = h[:, :w].to(self.device)
            self._head[idx] = 0
            self._fill[idx] = fill
            self._in[idx] = nin
            self._fmt[idx] = fmt
