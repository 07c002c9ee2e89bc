"""The expanded codecs without a GPU (afx/codecs.py and the host path of the fronts): the DVI4 decoder's known answer, its
agreement with CPython's audioop byte for byte, blocks that end on both clamps, the exact PCM decodes; and on host-only
scorers what a feed in a codec plans -- one "expand" op first, ingest / place rows that read the decoded zone as pcm_f32le
-- that a native feed plans what it always did, every refusal leaving the scorer unchanged, RTP's static audio types, and the
new entry point in the header, the library and the ctypes table."""
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


@pytest.fixture(scope="module")
def built():
    return packet_helpers.built()


def _block(pred, index, body):
    return bytes([(pred >> 8) & 255, pred & 255, index, 0]) + bytes(body)


# ---- the codecs ------------------------------------------------------------------------------------------------------------
def test_dvi4_known_answer_names_and_sample_counts():
    from afx import codecs
    from afx.ingest import ENCODINGS
    assert codecs.CODECS == ("dvi4", "pcm_s16be", "pcm_s24be", "pcm_u8") and ENCODINGS == ("pcm_f32le", "pcm_s16le", "mulaw", "alaw")
    assert len(codecs.STEP) == 89 and codecs.STEP[0] == 7 and codecs.STEP[88] == 32767 and codecs.IDX.tolist() == [-1, -1, -1, -1, 2, 4, 6, 8] * 2
    block = bytes.fromhex("fc1828007f19a3c0")
    assert codecs.dvi4_header(block) == (-1000, 40)
    want = [-369, -1726, -1144, -1672, -2473, -1454, -2646, -2486]
    got = codecs.dvi4_reference(block)
    assert got.dtype == np.int16 and got.tolist() == want
    ref = codecs.reference(block, "dvi4")
    assert ref.dtype == np.float32 and np.array_equal(ref, np.array(want, dtype=np.float32) / np.float32(32768))
    assert [codecs.samples(n, "dvi4") for n in (4, 5, 84)] == [0, 2, 160]
    assert (codecs.samples(6, "pcm_s16be"), codecs.samples(6, "pcm_s24be"), codecs.samples(6, "pcm_u8")) == (3, 2, 6)
    assert codecs.samples_each([84, 6, 6, 6], [0, 1, 2, 3]).tolist() == [160, 3, 2, 6]
    for nbytes, codec in ((3, "dvi4"), (5, "pcm_s16be"), (4, "pcm_s24be"), (4, "g722")):
        with pytest.raises(ValueError):
            codecs.samples(nbytes, codec)
    for bad in (bytes(3), _block(0, 89, b"\x00")):
        with pytest.raises(ValueError):
            codecs.dvi4_reference(bad)
    with pytest.raises(ValueError):
        codecs.reference(bytes(8), "g722")


def test_dvi4_decoder_and_encoder_equal_audioop_byte_for_byte():
    audioop = pytest.importorskip("audioop")
    from afx import codecs
    g = np.random.default_rng(1)
    bodies = [g.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in g.integers(0, 300, 40)]
    bodies += [bytes([v]) * 500 for v in (0x77, 0xFF, 0x00, 0x88, 0x7F, 0xF7)]
    for body in bodies:
        pred, index = int(g.integers(-32768, 32768)), int(g.integers(0, 89))
        lin, _ = audioop.adpcm2lin(body, 2, (pred, index))
        assert codecs.dvi4_reference(_block(pred, index, body)).astype("<i2").tobytes() == lin
    for n in (0, 2, 160, 1000):
        x = (g.integers(-32768, 32768, n) // g.choice([1, 8, 64])).astype(np.int16)
        state = None
        for cut in (x[:n // 4 * 2], x[n // 4 * 2:]):  # two blocks, the second continuing the first's state
            block, after = codecs.dvi4_encode(cut, state)
            body, want = audioop.lin2adpcm(cut.astype("<i2").tobytes(), 2, state)
            assert block[4:] == body and after == want
            assert codecs.dvi4_header(block) == (state or (0, 0)) and block[3] == 0
            assert codecs.dvi4_reference(block).astype("<i2").tobytes() == audioop.adpcm2lin(body, 2, state)[0]
            state = after
    with pytest.raises(ValueError):
        codecs.dvi4_encode(np.zeros(3, dtype=np.int16))


def test_dvi4_saturating_blocks_end_on_the_clamps():
    from afx import codecs

    def run(pred, index, code, n):
        """The decoder's state after n bytes of ``code``."""
        out = codecs.dvi4_reference(_block(pred, index, bytes([code]) * n))
        idx = index
        for c in [code >> 4, code & 15] * n:
            idx = min(max(idx + int(codecs.IDX[c]), 0), 88)
        return int(out[-1]), idx

    assert run(0, 80, 0x77, 64) == (32767, 88)
    assert run(0, 0, 0xFF, 200) == (-32768, 88)
    assert run(1234, 88, 0x00, 100)[1] == 0 and run(-1234, 88, 0x88, 100)[1] == 0
    up, down = codecs.dvi4_reference(_block(0, 88, b"\x00" * 100)), codecs.dvi4_reference(_block(0, 88, b"\x88" * 100))
    # code 0 adds step >> 3 and code 8 takes it, until each sits on its own clamp
    assert up[:13].tolist() == (-down[:13].astype(np.int32)).tolist() and up[0] == 32767 >> 3 and np.all(np.diff(up[:14]) > 0)
    assert set(up[13:].tolist()) == {32767} and set(down[13:].tolist()) == {-32768}
    # round trip: the decoder follows what the encoder tracked
    x = (8000 * np.sin(np.arange(400) / 9.0)).astype(np.int16)
    block, (pred, _) = codecs.dvi4_encode(x)
    y = codecs.dvi4_reference(block)
    assert int(y[-1]) == pred and np.abs(y[50:].astype(np.int32) - x[50:]).max() < 600


def test_pcm_codecs_are_exact_for_every_code_and_the_extremes():
    from afx import codecs
    u8 = codecs.reference(bytes(range(256)), "pcm_u8")
    assert u8.dtype == np.float32 and np.array_equal(u8.astype(np.float64), (np.arange(256) - 128) / 128.0)
    s16 = codecs.reference(bytes.fromhex("8000 ffff 0000 0001 7fff 0100"), "pcm_s16be")
    assert s16.tolist() == [-1.0, -1 / 32768, 0.0, 1 / 32768, 32767 / 32768, 256 / 32768]
    v = np.arange(-32768, 32768, dtype=np.int16)
    assert np.array_equal(codecs.reference(v.astype(">i2").tobytes(), "pcm_s16be"), v.astype(np.float32) / np.float32(32768))
    s24 = codecs.reference(bytes.fromhex("800000 ffffff 000000 000001 7fffff 010203"), "pcm_s24be")
    assert s24.dtype == np.float32 and s24.astype(np.float64).tolist() == [-1.0, -1 / 8388608, 0.0, 1 / 8388608, 8388607 / 8388608,
                                                                           0x010203 / 8388608]
    for name in ("pcm_u8", "pcm_s16be", "pcm_s24be", "dvi4"):
        assert codecs.reference(b"" if name != "dvi4" else bytes(4), name).shape == (0,)


# ---- what a feed in a codec plans ------------------------------------------------------------------------------------------
def _snap(ps):
    e = ps.export_slots(list(range(ps.S)))
    return [ps.pending, ps.samples_in, ps.samples_seen] + [e.tensors[k] for k in sorted(e.tensors)]


def _unchanged(before, ps):
    return all(torch.equal(a, b) for a, b in zip(before, _snap(ps)))


def test_packet_scorer_plans_one_expand_op_and_ingest_rows_in_the_decoded_zone(built):
    from afx import codecs
    from afx._lib import AfxError
    from afx.ingest import PacketScorer, expand_zone, payload
    ps = PacketScorer(_inner(3), 8000, "dvi4", max_pending=2)
    assert ps.encoding == "dvi4" and ps.L == 2
    pk = [bytes(4 + 80), _block(5, 88, bytes(3000)), bytes(4)]  # 160 samples, 6000 (more than a round takes), none
    idx, pay, (ops, counts, (head, fill, nin)) = ps._plan_feed(pk, [2, 0, 1])
    assert [op[0] for op in ops][:2] == ["expand", "ingest"] and [op[0] for op in ops].count("expand") == 1
    exp = ops[0]
    assert exp[1].dtype == np.int32 and exp[1].shape == (2, codecs.EXPAND_HDR) and exp[2] == 6000  # (the empty block has no row)
    # payloads at 0, 96 and 3104 of 3120 bytes; the zone is planned from there on, each block 16-byte aligned
    assert exp[1].tolist() == [[0, 84, 3120, 0], [96, 3004, 3120 + 640, 0]]
    first = ops[1][1]
    assert first[0].tolist()[:4] == [2, 3120, 160, 320] and first[1].tolist()[:2] == [0, 3760]
    done = 0
    for op in ops:  # the rows of slot 0 walk its decoded block 4 bytes a sample
        if op[0] == "ingest":
            for r in op[1].tolist():
                if r[0] == 0:
                    assert r[1] == 3760 + 4 * done
                    done += r[2]
    assert done == 6000 and nin == [6000, 0, 160] and counts == [0, 3, 0] and fill[0] == 0
    assert _unchanged(_snap(ps), ps) and ps.samples_in.tolist() == [0, 0, 0]  # planning changes nothing
    # where the zone comes to lie once the tables are known: behind them, every reader moved with it
    tables, zone = ps._stage(ops, [op[1] for op in ops], pay)
    up = 3120 + sum(-(-t.nbytes // 16) * 16 for t in tables)
    assert zone == 640 + 24000 and tables[0].tolist() == [[0, 84, up, 0], [96, 3004, up + 640, 0]]
    assert tables[1][0].tolist()[:2] == [2, up] and tables[1][1].tolist()[:2] == [0, up + 640]
    assert ops[0][1][0, 2] == 3120 and all(t.shape == op[1].shape for t, op in zip(tables, ops))  # (the plan is not edited)
    # the same three packets decoded on the host and fed as pcm_s16le: the same rounds, rows and counters but for the offsets
    ref = PacketScorer(_inner(3), 8000, "pcm_s16le", max_pending=2)
    _, _, (rops, rcounts, rafter) = ref._plan_feed([codecs.dvi4_reference(p).astype("<i2").tobytes() for p in pk], [2, 0, 1])
    assert [op[0] for op in rops] == [op[0] for op in ops[1:]] and rcounts == counts and rafter == (head, fill, nin)
    for a, b in zip(ops[1:], rops):
        assert np.array_equal(np.delete(a[1], 1, axis=1), np.delete(b[1], 1, axis=1))
    # a native scorer plans no expand op, and its staging is the tables as they are
    _, rpay, (rops, _, _) = ref._plan_feed([bytes(320)], [1])
    assert "expand" not in [op[0] for op in rops] and ref._stage(rops, [op[1] for op in rops], rpay)[1] == 0
    n, at, rows, zone = expand_zone([10, 20], [0, 16], 48, np.array([-1, -1]))
    assert rows is None and zone == 0 and at.tolist() == [0, 16]
    # refusals, each before anything changes
    before = _snap(ps)
    for bad in (bytes(3), _block(0, 89, bytes(8)), np.zeros(8, dtype=np.int16), "text"):
        with pytest.raises(ValueError):
            ps.feed([bytes(84), bad], [0, 1])
        assert _unchanged(before, ps)
    with pytest.raises(ValueError):
        ps.feed([bytes(4 + 8001)], [0], score=False)  # 16002 samples at 8 kHz are more than two hops at 16 kHz
    with pytest.raises(AfxError):  # valid, but there is no GPU behind this scorer
        ps.feed([bytes(84)], [0])
    assert _unchanged(before, ps)
    assert ps.feed([bytes(4), bytes(4)], [0, 1]).counts.tolist() == [0, 0]  # empty blocks complete nothing
    for codec, bad in (("pcm_s16be", bytes(3)), ("pcm_s24be", bytes(4))):
        other = PacketScorer(_inner(1), 8000, codec)
        with pytest.raises(ValueError):
            other.feed([bad], [0])
        assert payload(bytes(6), codec).size == 6
    for name in ("g722", "pcm_s16", "DVI4"):
        with pytest.raises(ValueError):
            PacketScorer(_inner(1), 8000, name)
    with pytest.raises(ValueError):
        payload(np.zeros(4, dtype=">i2"), "pcm_s16be")  # (a packet in a codec is bytes)


def test_mixed_packet_scorer_formats_in_codecs_say_encoding_zero(built):
    from afx.ingest import MixedPacketScorer
    formats = [(8000, "mulaw"), (8000, "dvi4"), (16000, "dvi4"), (44100, "pcm_s16be")]
    mp = MixedPacketScorer(_inner(4), formats)
    assert [t.encoding for t in mp._table] == [2, 0, 0, 0] and mp.formats == tuple(formats)
    mp.reset([0, 1, 2, 3], [0, 1, 2, 3])
    pk = [bytes(160), bytes(84), bytes(4 + 160), bytes(2 * 441)]
    idx, pay, (ops, counts, (head, fill, nin)) = mp._plan_feed(pk, [0, 1, 2, 3])
    assert [op[0] for op in ops][:2] == ["expand", "ingest"] and nin == [160, 160, 320, 441]
    front = 160 + 96 + 176 + 896
    assert ops[0][1].tolist() == [[160, 84, front, 0], [256, 164, front + 640, 0], [432, 882, front + 640 + 1280, 1]]
    rows = {r[0]: r for r in ops[1][1].tolist()}
    assert [rows[s][1] for s in range(4)] == [0, front, front + 640, front + 1920] and [rows[s][7] for s in range(4)] == [0, 1, 2, 3]
    before = _snap(mp)
    with pytest.raises(ValueError):
        mp.feed([bytes(160), _block(0, 99, b"")], [0, 1])
    with pytest.raises(ValueError):
        mp.feed([bytes(160), bytes(3)], [0, 3])
    assert _unchanged(before, mp)
    with pytest.raises(ValueError):
        MixedPacketScorer(_inner(1), [(8000, "g722")])


# ---- the jitter buffer -----------------------------------------------------------------------------------------------------
def _jitter(encoding, S=2, rate=8000, depth=480, **kw):
    from afx.jitter import JitterScorer
    return JitterScorer(_inner(S), rate, encoding, depth, **kw)


def _jsnap(js):
    e = js.export_slots(list(range(js.S)))
    return [js.pending, js.samples_in, js.buffered] + [e.tensors[k] for k in sorted(e.tensors)] + list(js.stats().values())


def test_jitter_feed_in_two_codecs_plans_one_expand_op_and_place_rows_of_encoding_zero(built):
    from afx.jitter import JitterScorer
    js = _jitter(("mulaw", "dvi4"))
    assert js.encodings == ("mulaw", "dvi4")
    # a DVI4 packet with timestamp t and B bytes covers [t, t + 2 (B - 4))
    plan, pay = js._plan_feed([bytes(160), bytes(84), bytes(84)], [0, 0, 1], [1000, 1160, 7], encodings=["mulaw", "dvi4", "dvi4"])
    kinds = [op[0] for op in plan.ops]
    assert kinds[:2] == ["expand", "place"] and kinds.count("expand") == 1 and [len(b) for b in pay] == [160, 84, 84]
    front = 160 + 96 + 96
    assert plan.ops[0][1].tolist() == [[160, 84, front, 0], [256, 84, front + 640, 0]] and plan.ops[0][2] == 160
    place = sorted(plan.ops[1][1].tolist())
    assert place == [[0, 0, 160, 0, 2], [0, front, 160, 160, 0], [1, front + 640, 160, 0, 0]]
    assert plan.book.hi.tolist() == [320, 160]
    js._commit(plan.book)
    # a DVI4 packet that overlaps what was received: the part already there is a duplicate, the rest is read from mid-block
    plan, _ = js._plan_feed([bytes(84)], [0], [1000 + 280], encodings=["dvi4"])
    rows = [r for op in plan.ops if op[0] == "place" for r in op[1].tolist()]
    assert rows == [[0, 96 + 4 * 40, 120, 320, 0]] and plan.book.dup[0] == 40
    tables, zone = js._stage(plan.ops, [op[1] for op in plan.ops], [bytes(84)])
    up = 96 + sum(-(-t.nbytes // 16) * 16 for t in tables)
    assert zone == 640 and tables[0].tolist() == [[0, 84, up, 0]] and tables[1].tolist() == [[0, up + 160, 120, 320, 0]]
    # native packets alone plan what they always did
    plan, _ = js._plan_feed([bytes(160)], [1], [167], encodings=["mulaw"])
    assert "expand" not in [op[0] for op in plan.ops] and [r for op in plan.ops if op[0] == "place" for r in op[1].tolist()] == [[1, 0, 160, 160, 2]]
    # one codec alone: four-column place rows, launched as encoding 0
    one = _jitter("dvi4")
    plan, _ = one._plan_feed([bytes(84)], [0], [0])
    assert one.encodings == ("dvi4",) and [op[0] for op in plan.ops][:2] == ["expand", "place"] and plan.ops[1][1].tolist() == [[0, 96, 160, 0]]
    # refusals
    before, book = _jsnap(js), js._b
    for args, kw in ((([bytes(3)], [0], [2000]), dict(encodings=["dvi4"])), (([_block(0, 89, bytes(4))], [0], [2000]), dict(encodings=["dvi4"])),
                     (([bytes(84)], [0], [2000]), dict(encodings=["pcm_s16be"])), (([bytes(84)], [0], [2000]), dict(encodings=["g722"]))):
        with pytest.raises(ValueError):
            js.feed(*args, **kw)
    assert js._b is book and all(torch.equal(a, b) for a, b in zip(before, _jsnap(js)))
    for bad in ("g722", ("mulaw", "g722"), ("dvi4", "dvi4")):
        with pytest.raises(ValueError):
            _jitter(bad)
    be = JitterScorer(_inner(1), 44100, "pcm_s16be", 2646)
    with pytest.raises(ValueError):
        be.feed([bytes(3)], [0], [0])
    plan, _ = be._plan_feed([bytes(2 * 882)], [0], [0])
    assert plan.ops[0][0] == "expand" and plan.ops[0][1].tolist() == [[0, 1764, 1776, 1]]


def test_static_audio_formats_and_what_feed_rtp_takes_without_payload_types(built):
    from afx import rtp
    from afx._lib import AfxError
    from afx.jitter import JitterScorer, MixedJitterScorer
    assert rtp.STATIC_PAYLOAD_TYPES == {0: "mulaw", 8: "alaw"}
    assert rtp.STATIC_AUDIO_FORMATS == {0: (8000, "mulaw"), 5: (8000, "dvi4"), 6: (16000, "dvi4"), 8: (8000, "alaw"),
                                        11: (44100, "pcm_s16be"), 16: (11025, "dvi4"), 17: (22050, "dvi4")}
    js = _jitter(("mulaw", "dvi4"), depth=0)
    plan, pay, _ = js._plan_rtp([_rtp(1, 800, pt=0, payload=bytes(160)), _rtp(2, 960, pt=5, payload=bytes(84))], [0, 0])
    assert plan.ops[0][0] == "expand" and [r[4] for r in plan.ops[1][1].tolist()] == [2, 0]
    for pt, rate in ((6, 16000), (16, 11025), (17, 22050)):
        assert JitterScorer(_inner(1), rate, "dvi4", 0)._plan_rtp([_rtp(1, 0, pt=pt, payload=bytes(84))], [0])[0].ops[0][0] == "expand"
    assert JitterScorer(_inner(1), 44100, "pcm_s16be", 0)._plan_rtp([_rtp(1, 0, pt=11, payload=bytes(64))], [0])[0].ops[0][0] == "expand"
    before = _jsnap(js)
    for pt, payload in ((6, bytes(84)), (8, bytes(160)), (10, bytes(64)), (11, bytes(64)), (96, bytes(84)), (5, bytes(3)),
                        (5, _block(0, 89, bytes(4)))):  # another rate's type, a type not listed, stereo, unknown; malformed
        with pytest.raises(ValueError):
            js.feed_rtp([_rtp(1, 800, pt=pt, payload=payload)], [0])
    assert all(torch.equal(a, b) for a, b in zip(before, _jsnap(js)))
    with pytest.raises(ValueError, match="payload type 5"):  # a scorer that does not list dvi4 refuses it as before
        _jitter("mulaw").feed_rtp([_rtp(1, 800, pt=5, payload=bytes(84))], [0])
    with pytest.raises(ValueError, match="payload type 11"):  # little-endian L16 is not what PT 11 carries
        JitterScorer(_inner(1), 44100, "pcm_s16le", 0).feed_rtp([_rtp(1, 0, pt=11, payload=bytes(64))], [0])
    with pytest.raises(AfxError):  # accepted and planned
        js.feed_rtp([_rtp(1, 800, pt=5, payload=bytes(84))], [0])
    mx = MixedJitterScorer(_inner(4), [(8000, "mulaw"), (8000, "dvi4"), (16000, "dvi4"), (44100, "pcm_s16be")], 60)
    mx.reset([1], 16000)
    mx.reset([2], 44100)
    d = [_rtp(1, 0, pt=0, payload=bytes(160)), _rtp(1, 0, pt=6, payload=bytes(4 + 160)), _rtp(1, 0, pt=11, payload=bytes(2 * 882)), _rtp(1, 0, pt=5, payload=bytes(84))]
    plan, pay, _ = mx._plan_rtp(d, [0, 1, 2, 3])
    assert plan.ops[0][0] == "expand" and plan.ops[0][1][:, 3].tolist() == [0, 1, 0] and plan.ops[0][2] == 882
    assert sorted((r[0], r[4], r[5]) for r in plan.ops[1][1].tolist()) == [(0, 2, 0), (1, 0, 1), (2, 0, 2), (3, 0, 0)]
    for pt, slot in ((5, 1), (6, 0), (11, 0), (10, 2), (16, 0), (17, 1)):
        with pytest.raises(ValueError):
            mx.feed_rtp([_rtp(1, 0, pt=pt, payload=bytes(84))], [slot])
    assert not mx._b.started.any()


def test_a_state_does_not_say_which_codec_it_was_fed_in(built):
    a, b = _jitter("dvi4"), _jitter("pcm_s16le")
    st = a.export_slots([0, 1])
    assert st.meta == b.export_slots([0, 1]).meta and "encoding" not in st.meta
    b.import_slots([1, 0], st)
    a.import_slots([0, 1], b.export_slots([0, 1]))


def test_expand_entry_point_is_in_header_library_and_ctypes_table(built):
    src = open(os.path.join(ROOT, "include", "afx.h")).read()
    assert all(w in src for w in ("dvi4", "pcm_s16be", "pcm_s24be", "pcm_u8"))
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = ctypes.CDLL(built.LIB_PATH)
    name = "afx_k_payload_expand"
    assert re.search(r"\b%s\s*\(" % name, src) and hasattr(lib, name) and name in built.SIGNATURES
    l = built.lib()
    buf = (ctypes.c_char * 64)()
    hdr = (ctypes.c_int * 4)()
    for args in ((None, 64, hdr, 1, 1), (buf, 64, None, 1, 1), (buf, 0, hdr, 1, 1), (buf, 64, hdr, 0, 1), (buf, 64, hdr, 65536, 1),
                 (buf, 64, hdr, 1, -1), (buf, 64, hdr, 1, 17)):  # each refused on the host: nothing is launched
        assert l.afx_k_payload_expand(*args, None) != 0 and b"afx_k_payload_expand" in l.afx_last_error()
