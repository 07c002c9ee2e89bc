"""Several formats on one packet front (afx/ingest.py MixedPacketScorer, afx_k_ingest_mixed) and several encodings in one
jitter buffer (afx/jitter.py, afx_k_jitter_place_mixed), without a GPU: a mixed feed plans, for every slot, the rows the
single-format ``PacketScorer`` plans for that slot alone (column 7 apart: the format index); every refusal leaves a
host-only scorer unchanged; the state an export adds and what an import refuses; the new entry points in the header, the
library and the ctypes table with every host refusal of ``afx_k_ingest_mixed``; and the place rows of a jitter feed over
packets of mixed encodings."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import packet_helpers
from oracle.jitter import rtp as _rtp
from packet_helpers import inner as _inner

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 4000
FORMATS = [(8000, "mulaw"), (11025, "pcm_s16le"), (16000, "pcm_f32le"), (48000, "pcm_s16le")]
BPS = {"pcm_f32le": 4, "pcm_s16le": 2, "mulaw": 1, "alaw": 1}


@pytest.fixture(scope="module")
def built():
    return packet_helpers.built()


def _mixed(S=4, formats=FORMATS, max_pending=2, spread=True):
    from afx.ingest import MixedPacketScorer
    ms = MixedPacketScorer(_inner(S), formats, max_pending)
    if spread:  # slot s in format s mod len(formats)
        ms.reset(list(range(S)), [s % len(formats) for s in range(S)])
    return ms


def _plain(S, rate, encoding, max_pending=2):
    from afx.ingest import PacketScorer
    return PacketScorer(_inner(S), rate, encoding, max_pending)


def _snap(ps):
    e = ps.export_slots(list(range(ps.S)))
    out = [ps.pending, ps.samples_in, ps.samples_seen, ps.scorer.samples_seen] + [e.tensors[k] for k in sorted(e.tensors)]
    return out + ([ps.format_of, ps.rates, ps.delays] if hasattr(ps, "format_of") else [])


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a, b))


# ---- planning ------------------------------------------------------------------------------------------------------------
def test_a_mixed_feed_plans_each_slots_single_format_rows():
    ms = _mixed()
    assert ms.format_of.tolist() == [0, 1, 2, 3] and ms.rates.tolist() == [8000, 11025, 16000, 48000]
    assert ms.delays.tolist() == [20.0, _plain(1, 11025, "mulaw").delay, 0.0, 10.0] and ms.ring_len == 3 * H
    singles = [_plain(4, r, e) for r, e in FORMATS]
    # every slot some way into its stream: N inputs received, the outputs they made pending (less than a hop) at some head
    for s, (N, head) in enumerate(((1234, 0), (777, 5000), (40, 11999), (100001, 8000))):
        L, M = singles[s].L, singles[s].M
        for ps in (ms, singles[s]):
            ps._in[s], ps._head[s] = N, head
            ps._fill[s] = -(-N * L // M) % H
    before = _snap(ms)
    room = {s: (3 * H - int(ms._fill[s])) * singles[s].M // singles[s].L for s in range(4)}
    order = [2, 0, 3, 1]  # shuffled: slot 2 (identity) gets more than the ring takes at once, 0 nothing, 3 one sample, 1 221
    sizes = {2: room[2] + 2 * H + 17, 0: 0, 3: 1, 1: 221}
    offs = {2: 0, 0: 4 * sizes[2], 3: 4 * sizes[2], 1: 4 * sizes[2] + 16}
    assert sizes[2] > room[2]
    ops, counts, (head, fill, nin) = ms._plan(order, [sizes[s] for s in order], [offs[s] for s in order], score=True)
    assert _same(before, _snap(ms))  # planning changes nothing
    ingests = [op for op in ops if op[0] == "ingest"]
    assert len(ingests) >= 2 and all(op[1].dtype == np.int32 and op[1].shape[1] == 8 for op in ingests)
    assert [op[2] for op in ingests] == [int(op[1][:, 3].max()) for op in ingests]
    assert sorted(ingests[0][1][:, 0].tolist()) == [1, 2, 3]  # one launch for the three slots that brought samples
    for i, s in enumerate(order):
        one_ops, one_counts, (h1, f1, n1) = singles[s]._plan([s], [sizes[s]], [offs[s]], score=True)
        want = [op[1][0] for op in one_ops if op[0] == "ingest"]
        got = [row for op in ingests for row in op[1] if row[0] == s]
        assert len(got) == len(want) and (len(got) > 0) == (sizes[s] > 0)
        for g, w in zip(got, want):
            assert g[:7].tolist() == w[:7].tolist() and w[7] == 0 and g[7] == s  # (slot s is in format s)
        assert counts[i] == one_counts[0] and (head[s], fill[s], nin[s]) == (h1[s], f1[s], n1[s])
        assert nin[s] == int(ms._in[s]) + sizes[s]
    assert counts[0] >= 2 and len([r for op in ingests for r in op[1] if r[0] == 2]) >= 2  # the long packet took two rounds
    # the pops of a round are shared: every slot that holds a whole hop after a round's ingest is in that round's table
    pops = [op for op in ops if op[0] == "pop"]
    assert sum(len(op[2]) for op in pops) == sum(counts)


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_leave_a_mixed_host_scorer_unchanged(built):
    from afx._lib import AfxError
    from afx.ingest import MAX_FORMATS, MixedPacketScorer
    sc = _inner(2)
    seventeen = [(8000 + 100 * i, "mulaw") for i in range(17)]
    assert MAX_FORMATS == 16 and len(MixedPacketScorer(sc, seventeen[:16]).formats) == 16
    for bad in ([], seventeen, [(8000, "mulaw"), (8000, "mulaw")], [(7999, "mulaw")], [(8000.5, "mulaw")], [(8000, "g722")],
                [8000], [(8000,)], "mulaw", 8000, None, [(8000, "mulaw", 1)]):
        with pytest.raises(ValueError):
            MixedPacketScorer(sc, bad)
    for kw in (dict(max_pending=0), dict(max_pending=1.5)):
        with pytest.raises(ValueError):
            MixedPacketScorer(sc, FORMATS, **kw)
    assert sc.samples_seen.tolist() == [0, 0]
    fresh = MixedPacketScorer(sc, FORMATS)
    assert fresh.format_of.tolist() == [0, 0] and fresh.formats == tuple(FORMATS) and fresh.layer == "front"
    # formats that share a rate share one Resampler
    two = MixedPacketScorer(sc, [(8000, "mulaw"), (8000, "alaw"), (16000, "pcm_s16le")])
    assert len(two._rs) == 2 and two._table[0].taps == two._table[1].taps and two._table[2].taps is None and two.Hs == two._rs[8000].T - 1

    ms = _mixed(S=4, max_pending=4)
    st = ms.export_slots([0])  # a session with pending samples in slot 0 (mulaw, 8 kHz): 50 inputs made 100 outputs
    st.tensors["ingest_fill"], st.tensors["ingest_in"] = torch.tensor([100]), torch.tensor([50])
    st.tensors["ingest_pending"][0, :100] = torch.arange(100.0)
    ms.import_slots([0], st)
    before = _snap(ms)
    assert before[0].tolist() == [100, 0, 0, 0] and before[1].tolist() == [50, 0, 0, 0]
    for slots, fm in (([0], 4), ([0], -1), ([0, 1], [0]), ([0], [0, 1]), ([1], (8000, "alaw")), ([1], (8000,)), ([1], "mulaw"),
                      ([1], 1.0), ([1], True), ([1, 1], 0), ([4], 0)):
        with pytest.raises(ValueError):
            ms.reset(slots, fm)
        assert _same(before, _snap(ms))
    three = b"abc"
    with pytest.raises(ValueError):  # 3 bytes split a sample of slot 1's pcm_s16le; slot 0's mulaw would take them
        ms.feed([three, three], [0, 1])
    assert _same(before, _snap(ms))
    with pytest.raises(ValueError):  # and of slot 2's pcm_f32le
        ms.feed([three], [2])
    with pytest.raises(AfxError):  # the same 3 bytes are three mu-law samples: planned, and refused only for want of a GPU
        ms.feed([three, b"abcd"], [0, 1])
    assert _same(before, _snap(ms))
    # score=False overflow is judged with the slot's own L / M: 4 hops of room, 100 taken in slot 0
    n8 = (4 * H - 100) // 2  # 8 kHz: two outputs per input
    n48 = 4 * H * 3  # 48 kHz: one output per three inputs
    for pk, slot in ((bytes(n8 + 1), 0), (bytes(2 * (n48 + 1)), 3), (bytes(4 * (4 * H + 1)), 2)):
        with pytest.raises(ValueError):
            ms.feed([pk], [slot], score=False)
        assert _same(before, _snap(ms))
    for args in (([three], [0, 1]), ([three, three], [0, 0]), ([three], [4]), (three, [0])):
        with pytest.raises(ValueError):
            ms.feed(*args)
    with pytest.raises(AfxError):  # valid (what fits exactly), but there is no GPU behind this scorer: nothing changes either
        ms.feed([bytes(n8), bytes(2 * n48)], [0, 3], score=False)
    assert _same(before, _snap(ms))
    res = ms.feed([b"", bytearray(), b""], [3, 0, 1])  # empty packets are legal and complete nothing
    assert res.counts.tolist() == [0, 0, 0] and res.scores.numel() == 0
    assert ms.drain().counts.tolist() == [0, 0, 0, 0]
    ms.reset([0])  # None keeps the format
    assert ms.pending.tolist() == [0, 0, 0, 0] and ms.format_of.tolist() == [0, 1, 2, 3]
    ms.reset([3, 0], [(8000, "mulaw"), 3])  # pairs and indices, one per named slot, in the order named
    assert ms.format_of.tolist() == [3, 1, 2, 0] and ms.rates.tolist() == [48000, 11025, 16000, 8000]
    ms.reset([1, 2], (48000, "pcm_s16le"))
    assert ms.format_of.tolist() == [3, 3, 3, 0]


# ---- state -----------------------------------------------------------------------------------------------------------------
def test_mixed_state_keys_meta_and_import_refusals(built):
    from afx.ingest import INGEST_FORMAT, MixedPacketScorer
    from afx.streaming import ResamplingScorer, StreamState
    ms = _mixed(formats=FORMATS + [(96000, "pcm_s16le")], max_pending=3)  # slots 0..3 in the first four formats
    T = {r: x.T for r, x in ms._rs.items()}
    assert ms.Hs == T[96000] - 1 == 120 and tuple(ms.hist.shape) == (4, ms.Hs) and T[16000] == 1
    st = ms.export_slots([3, 0, 2])
    assert set(st.tensors) == {"samples", "ingest_pending", "ingest_fill", "ingest_in", "resample_hist", "ingest_rate"}
    assert tuple(st.tensors["ingest_pending"].shape) == (3, 3 * H) and tuple(st.tensors["resample_hist"].shape) == (3, ms.Hs)
    assert st.tensors["ingest_rate"].dtype == torch.int64 and st.tensors["ingest_rate"].tolist() == [48000, 8000, 16000]
    assert st.meta["resampler"] == "kaiser5-hl10" and st.meta["ingest"] == INGEST_FORMAT and st.meta["ingest_mixed"] == 1
    assert "input_rate" not in st.meta and "encoding" not in st.meta and ms.state_meta() == st.meta
    # a history as a session at 48 kHz would leave it: its own T - 1 columns, zeros beyond
    own = T[48000] - 1
    assert own < ms.Hs
    st.tensors["resample_hist"][0, :own] = torch.arange(1.0, own + 1)
    st2 = StreamState.from_state_dict(st.to("cpu").state_dict())
    # another scorer: formats in another order, another S, an encoding the source did not have at that rate
    other = MixedPacketScorer(_inner(5), [(16000, "pcm_s16le"), (48000, "pcm_f32le"), (8000, "alaw"), (48000, "pcm_s16le")], 4)
    other.import_slots([4, 1, 0], st2)
    assert other.format_of.tolist() == [0, 2, 0, 0, 1]  # by default the first format at the session's rate
    back = other.export_slots([4, 1, 0])
    assert back.tensors["ingest_rate"].tolist() == [48000, 8000, 16000]
    assert tuple(back.tensors["resample_hist"].shape) == (3, other.Hs)
    assert torch.equal(back.tensors["resample_hist"][0, :own], st.tensors["resample_hist"][0, :own])
    assert not back.tensors["resample_hist"][0, own:].any() and not back.tensors["resample_hist"][1:].any()
    other.import_slots([2, 3, 4], st2, formats=[3, (8000, "alaw"), 0])
    assert other.format_of.tolist() == [0, 2, 3, 2, 0]
    keep = _snap(other)
    narrow = MixedPacketScorer(_inner(3), [(48000, "pcm_s16le"), (16000, "pcm_f32le")])  # Hs = 48 kHz's own T - 1
    refused = [(other, [0, 1, 2], st2, [1, 2, 3]),  # a format at another rate than the session's (16 kHz into 48 kHz)
               (other, [0, 1, 2], st2, [1, 0, 0]),
               (other, [0, 1, 2], st2, [1, 2]), (other, [0, 1, 2], st2, 4), (other, [0, 1], st2, None), (other, [0, 0, 1], st2, None),
               (narrow, [0, 1, 2], st2, None)]  # 8 kHz is none of narrow's rates
    for dst, slots, state, fm in refused:
        with pytest.raises(ValueError):
            dst.import_slots(slots, state, fm)
    assert _same(keep, _snap(other))
    one = ms.export_slots([3])  # the 48 kHz session alone: as wide as ms.Hs, zeros beyond its own -> fits narrow
    one.tensors["resample_hist"][0, :own] = 1.0
    narrow.import_slots([1], one)
    assert narrow.format_of.tolist() == [0, 0, 0] and bool((narrow.hist[1] == 1.0).all())
    keep = _snap(narrow)
    one.tensors["resample_hist"][0, own] = 0.5  # a non-zero column beyond the session's own, wider than narrow's Hs
    with pytest.raises(ValueError):
        narrow.import_slots([2], one)
    short = StreamState(one.meta, one.seen, dict(one.tensors, resample_hist=one.tensors["resample_hist"][:, :own - 1].clone()))
    with pytest.raises(ValueError):
        narrow.import_slots([2], short)
    for key, val in (("resampler", "other"), ("ingest", INGEST_FORMAT + 1), ("hop", 2000), ("ingest_mixed", 2)):
        with pytest.raises(ValueError):
            narrow.import_slots([2], StreamState(dict(st.meta, **{key: val}), st.seen[:1], {k: v[:1] for k, v in st.tensors.items()}))
    bad_rate = StreamState(st.meta, st.seen[:1], {k: (v[:1].to(torch.int32) if k == "ingest_rate" else v[:1]) for k, v in st.tensors.items()})
    wrapped = ResamplingScorer(_inner(1), 48000)
    for foreign in (bad_rate, _inner(1).export_slots([0]), wrapped.export_slots([0]), st.tensors, None):
        with pytest.raises(ValueError):
            narrow.import_slots([2], foreign)
    full = ms.export_slots([3])  # counters that contradict each other (judged with the session's own L / M); too much pending
    full.tensors["ingest_fill"], full.tensors["ingest_in"] = torch.tensor([2 * H + 1]), torch.tensor([3 * (2 * H + 1) - 3])
    with pytest.raises(ValueError):
        narrow.import_slots([2], full)
    full.tensors["ingest_in"] = torch.tensor([3 * (2 * H + 1)])
    with pytest.raises(ValueError):
        MixedPacketScorer(_inner(1), FORMATS, max_pending=2).import_slots([0], full)
    assert _same(keep, _snap(narrow))
    narrow.import_slots([2], full)
    assert narrow.pending.tolist() == [0, 0, 2 * H + 1] and narrow.samples_in.tolist() == [0, 0, 3 * (2 * H + 1)]

    # a plain PacketScorer's state imports (the migration path); a mixed state into a plain PacketScorer does not
    plain = _plain(2, 48000, "pcm_s16le", max_pending=3)
    pst = plain.export_slots([1])
    pst.tensors["ingest_fill"], pst.tensors["ingest_in"] = torch.tensor([7]), torch.tensor([21])
    pst.tensors["ingest_pending"][0, :7] = torch.arange(7.0)
    pst.tensors["resample_hist"][0] = torch.arange(float(own))
    assert tuple(pst.tensors["resample_hist"].shape) == (1, own) and pst.meta["input_rate"] == 48000
    ms.import_slots([1], pst)  # slot 1 was at 11 025 Hz: it continues the session at 48 kHz
    assert ms.format_of.tolist() == [0, 3, 2, 3] and ms.pending.tolist() == [0, 7, 0, 0] and ms.samples_in.tolist() == [0, 21, 0, 0]
    assert torch.equal(ms.hist[1, :own], torch.arange(float(own))) and not ms.hist[1, own:].any()
    with pytest.raises(ValueError):
        MixedPacketScorer(_inner(1), [(8000, "mulaw")]).import_slots([0], pst)
    with pytest.raises(ValueError):
        ms.import_slots([0], pst, formats=0)
    with pytest.raises(ValueError):
        plain.import_slots([0], ms.export_slots([1]))


# ---- entry points ------------------------------------------------------------------------------------------------------------
def test_mixed_entry_points_are_in_header_library_and_ctypes_table(built):
    src = open(os.path.join(ROOT, "include", "afx.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = ctypes.CDLL(built.LIB_PATH)
    for name in ("afx_k_ingest_mixed", "afx_k_jitter_place_mixed", "afx_k_ingest", "afx_k_jitter_place"):
        assert re.search(r"\b%s\s*\(" % name, src) and hasattr(lib, name) and name in built.SIGNATURES
    assert re.search(r"\bafx_ingest_format\b", src)
    l = built.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def table(*fm):  # (taps, encoding, L, M, T)
        t = (built.IngestFormat * max(len(fm), 1))()
        for e, f in zip(t, fm):
            e.taps, e.encoding, e.L, e.M, e.T = f
        return ctypes.cast(t, ctypes.c_void_p), t

    def refused(word, fm, most, n=None, stage=p, hdr=p, hist=p, Hs=60, ring=p, ring_len=16, rows=1):
        tp, keep = table(*fm)
        mo = (ctypes.c_int * 17)(*most)
        rc = l.afx_k_ingest_mixed(stage, 64, hdr, rows, tp, len(fm) if n is None else n, ctypes.cast(mo, ctypes.c_void_p), hist, Hs,
                                  ring, 1, ring_len, None)
        assert rc != 0 and b"ingest_mixed" in l.afx_last_error() and word in l.afx_last_error(), l.afx_last_error()

    ident, up2, f48 = (None, 0, 1, 1, 1), (p.value, 2, 2, 1, 41), (p.value, 1, 1, 3, 61)
    # refused on the host: nothing is launched (there is no GPU here to launch on)
    assert l.afx_k_ingest_mixed(None, 0, None, 1, None, 1, None, None, 0, None, 1, 1, None) != 0 and b"ingest_mixed" in l.afx_last_error()
    refused(b"1 to 16 formats", [ident], [1], n=0)
    refused(b"1 to 16 formats", [ident] * 17, [1] * 17)
    refused(b"encoding", [ident, (None, 4, 1, 1, 1)], [1, 1])
    refused(b"encoding", [(None, -1, 1, 1, 1)], [1])
    refused(b"filter shape", [up2, (p.value, 0, 0, 1, 41)], [1, 1])
    refused(b"filter shape", [(p.value, 0, 2, 1, 0)], [1])
    refused(b"filter shape", [(None, 0, 2, 1, 41)], [1])  # no taps is the identity
    refused(b"256 carried", [(p.value, 0, 2, 1, 258)], [1], Hs=300)
    refused(b"ratio above 12", [up2, (p.value, 0, 1, 16, 257)], [1, 0], Hs=400)  # (refused whether or not a row uses it)
    refused(b"null", [up2], [1], ring=None)
    refused(b"null", [up2], [1], stage=None)
    refused(b"null", [up2], [1], hdr=None)
    refused(b"fit", [up2, f48], [1, 17])  # max_out beyond the ring
    refused(b"fit", [up2], [-1])
    refused(b"narrower", [up2, f48], [1, 1], Hs=59)  # Hs below 48 kHz's T - 1 = 60
    refused(b"null history", [ident, up2], [1, 1], hist=None)
    refused(b"rows", [up2], [1], rows=0)
    refused(b"rows", [up2], [1], rows=65536)
    assert l.afx_k_jitter_place_mixed(None, 0, None, 1, 1, None, 1, 1, None) != 0 and b"jitter_place_mixed" in l.afx_last_error()
    assert l.afx_k_jitter_place_mixed(p, 64, p, 1, 17, p, 1, 16, None) != 0 and b"fit" in l.afx_last_error()  # max_n > J
    assert l.afx_k_jitter_place_mixed(p, 64, p, 0, 1, p, 1, 16, None) != 0 and b"rows" in l.afx_last_error()


# ---- jitter ----------------------------------------------------------------------------------------------------------------
def _jitter(encoding, S=2, depth=160, **kw):
    from afx.jitter import JitterScorer
    return JitterScorer(_inner(S), 8000, encoding, depth, **kw)


def test_jitter_place_rows_carry_each_packets_encoding(built):
    from afx.ingest import ENCODINGS
    from afx.jitter import PLACE_HDR, PLACE_MIXED_HDR
    assert (PLACE_HDR, PLACE_MIXED_HDR) == (4, 5)
    js = _jitter(("mulaw", "pcm_s16le", "alaw", "pcm_f32le"))
    assert js.encodings == ("mulaw", "pcm_s16le", "alaw", "pcm_f32le") and js.encoding == "mulaw"
    # four packets of 160 samples: slot 0 in order in three encodings, slot 1 one packet; then one that overlaps what slot 0 holds
    encs = ["mulaw", "pcm_s16le", "pcm_f32le", "alaw"]
    pk = [bytes(160 * BPS[e]) for e in encs]
    plan, pay = js._plan_feed(pk, [0, 0, 1, 0], [1000, 1160, 50, 1320], encodings=encs)
    place = [op for op in plan.ops if op[0] == "place"]
    assert len(place) == 1 and place[0][1].dtype == np.int32 and place[0][1].shape == (4, 5) and place[0][2] == 160
    offs = [0, 160, 160 + 320, 160 + 320 + 640]
    want = {(0, 0, 160, 0, 2), (0, 160, 160, 160, 1), (1, 480, 160, 0, 0), (0, 1120, 160, 320, 3)}
    assert {tuple(r) for r in place[0][1].tolist()} == want and [len(b) for b in pay] == [160, 320, 640, 160]
    assert all(tuple(r)[4] == ENCODINGS.index(e) and tuple(r)[1] == o for r, e, o in zip(sorted(place[0][1].tolist(), key=lambda r: r[1]), encs, offs))
    js._commit(plan.book)
    # a late overlapping packet in pcm_s16le: the part already received is dropped, the byte offset of the rest counts 2-byte samples
    plan, _ = js._plan_feed([bytes(2 * 100), bytes(40)], [0, 1], [1000 + 420, 50 + 200], encodings=["pcm_s16le", "alaw"])
    rows = [r for op in plan.ops if op[0] == "place" for r in op[1].tolist()]
    assert [0, 2 * 60, 40, 480 % js.J, 1] in rows and [1, 208, 40, 200, 3] in rows and len(rows) == 2
    # refusals: an encoding that is not listed, a wrong count, bytes that split a sample of the packet's own encoding
    book = js._b
    for args, kw in ((([bytes(4)], [0], [2000]), dict(encodings=["g722"])), (([bytes(4)], [0], [2000]), dict(encodings=["alaw", "alaw"])),
                     (([bytes(3)], [0], [2000]), dict(encodings=["pcm_s16le"])), (([bytes(6)], [0], [2000]), dict(encodings=["pcm_f32le"])),
                     (([bytes(4)], [0], [2000]), dict(encodings="alaw"))):
        with pytest.raises(ValueError):
            js.feed(*args, **kw)
    assert js._b is book
    assert js._plan_feed([bytes(3)], [0], [2000], encodings=["alaw"])[0].ops  # (the same 3 bytes are three A-law samples)
    with pytest.raises(ValueError):
        _jitter(("mulaw", "mulaw"))
    with pytest.raises(ValueError):
        _jitter(("mulaw", "g722"))
    with pytest.raises(ValueError):
        _jitter(())
    # one name behaves as before: four-column rows for afx_k_jitter_place, and no other encoding per packet
    one = _jitter("alaw")
    plan, _ = one._plan_feed([bytes(160)], [0], [0])
    assert one.encodings == ("alaw",) and [op[1].shape for op in plan.ops if op[0] == "place"] == [(1, 4)]
    plan, _ = one._plan_feed([bytes(160)], [0], [0], encodings=["alaw"])
    assert [op[1].tolist() for op in plan.ops if op[0] == "place"] == [[[0, 0, 160, 0]]]
    with pytest.raises(ValueError):
        one._plan_feed([bytes(160)], [0], [0], encodings=["mulaw"])
    # a tuple of one name takes the per-row entry too
    plan, _ = _jitter(("alaw",))._plan_feed([bytes(160)], [0], [0])
    assert [op[1].tolist() for op in plan.ops if op[0] == "place"] == [[[0, 0, 160, 0, 3]]]


def test_feed_rtp_takes_every_listed_payload_type(built):
    from afx._lib import AfxError
    both, mu = _jitter(("mulaw", "alaw"), depth=0), _jitter("mulaw", depth=0)
    d0, d8 = _rtp(1, 800, pt=0, payload=bytes(160)), _rtp(2, 960, pt=8, payload=bytes(160))
    seen = []
    orig = both.feed
    both.feed = lambda *a, **kw: seen.append(kw["encodings"]) or orig(*a, **kw)
    with pytest.raises(AfxError):  # accepted and planned (there is no GPU behind this scorer to run it)
        both.feed_rtp([d0, d8], [0, 0])
    assert seen == [["mulaw", "alaw"]]
    plan, _ = both._plan_feed([bytes(160), bytes(160)], [0, 0], [800, 960], encodings=["mulaw", "alaw"])
    assert [r[4] for op in plan.ops if op[0] == "place" for r in op[1].tolist()] == [2, 3]
    with pytest.raises(ValueError, match="payload type 8"):
        mu.feed_rtp([d8], [0])
    with pytest.raises(ValueError, match="payload type 8"):
        mu.feed_rtp([d0, d8], [0, 0])
    assert mu.buffered.tolist() == [0, 0] and not mu._b.started.any()
    with pytest.raises(ValueError, match="payload type 96"):
        both.feed_rtp([_rtp(1, 800, pt=96, payload=bytes(320))], [0])
    with pytest.raises(AfxError):  # a dynamic type mapped to a listed encoding is taken; to one not listed, refused
        both.feed_rtp([_rtp(1, 800, pt=96, payload=bytes(160))], [1], payload_types={96: "alaw"})
    with pytest.raises(ValueError, match="payload type 96"):
        both.feed_rtp([_rtp(1, 800, pt=96, payload=bytes(320))], [1], payload_types={96: "pcm_s16le"})
    with pytest.raises(AfxError):
        mu.feed_rtp([d0], [0])


# ---- the stack -----------------------------------------------------------------------------------------------------------------
class _Model:
    def forward(self, batch):
        return torch.zeros(batch.shape[0], 2)

    def state_dict(self):
        return {"w": torch.ones(3)}


def test_a_mixed_front_goes_around_the_whole_stack(built):
    from afx.cascade import CascadePolicy, CascadeScorer
    from afx.evidence import EvidencePolicy, EvidenceScorer
    from afx.ingest import MixedPacketScorer, PacketScorer
    from afx.quality import QualityPolicy, QualityScorer
    from afx.vad import GatedScorer
    from afx.verdict import VerdictPolicy, VerdictScorer

    def stack(S):
        return GatedScorer(EvidenceScorer(VerdictScorer(QualityScorer(CascadeScorer(_inner(S), _Model(), CascadePolicy(0.0, 2)), QualityPolicy()),
                                                        VerdictPolicy(0.0, 0.5, verifier_enter=-0.5)), EvidencePolicy()))

    a = MixedPacketScorer(stack(3), FORMATS)
    assert a.layer == "front" and a.S == 3 and a.hop == H and a.state_meta() == dict(a.scorer.state_meta(), **a._meta())
    a.reset([2, 0], [3, (11025, "pcm_s16le")])
    assert a.format_of.tolist() == [1, 0, 3]
    st = a.export_slots([0, 2])
    assert st.tensors["ingest_rate"].tolist() == [11025, 48000] and set(a.scorer.export_slots([0, 2]).tensors) < set(st.tensors)
    b = MixedPacketScorer(stack(2), list(reversed(FORMATS)))
    b.import_slots([1, 0], st)
    assert b.format_of.tolist() == [0, 2] and b.rates.tolist() == [48000, 11025]
    with pytest.raises(ValueError):  # a front is the outermost layer: no layer goes around it
        GatedScorer(a)
    with pytest.raises(ValueError):  # and a plain packet front does not take a mixed state
        PacketScorer(stack(2), 48000, "pcm_s16le").import_slots([0], a.export_slots([2]))
