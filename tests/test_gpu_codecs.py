"""The expanded codecs on the GPU (afx/codecs.py, afx_k_payload_expand): the kernel alone over one ragged launch of DVI4
blocks on, under and over the 64-code step, on both clamps, and PCM rows, with bad rows that leave their destination's
poison; then every front in a codec against the same front in a native encoding fed ``codecs.reference`` of the same packets
in the same calls.  Every equality is bit for bit."""
import random

import numpy as np
import pytest
import torch

from oracle.jitter import rtp
from packet_helpers import tap as _tap

pytestmark = pytest.mark.gpu

H = 4000


def _same_hops(a, b, least=1):
    for ga, gb in zip(a.got, b.got):
        assert len(ga) == len(gb)
        if ga:
            assert torch.equal(torch.cat(ga), torch.cat(gb))
    assert sum(map(len, a.got)) >= least


def _speech(n, g, level=6000.0):
    """n int16 samples of a wandering tone with noise: what an ADPCM encoder follows without sitting on its clamps."""
    t = np.arange(n)
    x = level * np.sin(2 * np.pi * t * g.uniform(0.01, 0.08)) + 0.1 * level * g.standard_normal(n)
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def _dvi4(n, g, state=None):
    """One DVI4 packet of n (even) samples: encoded speech, or now and then random codes behind a random header."""
    from afx.codecs import dvi4_encode
    if g.random() < 0.25:
        pred, idx = int(g.integers(-32768, 32768)), int(g.integers(0, 89))
        return bytes([(pred >> 8) & 255, pred & 255, idx, 0]) + g.integers(0, 256, n // 2, dtype=np.uint8).tobytes()
    return dvi4_encode(_speech(n, g), state)[0]


def _s16le(block):
    from afx.codecs import dvi4_reference
    return dvi4_reference(block).astype("<i2").tobytes()


# ---- the kernel alone ------------------------------------------------------------------------------------------------------
def test_one_ragged_expand_launch_equals_the_reference_and_bad_rows_write_nothing():
    from afx import codecs
    from afx._lib import call_on, check, lib
    from afx.ingest import _at, layout, pack
    g = np.random.default_rng(7)
    rows = []  # (payload bytes, codec number, what its destination must hold: the samples, or None for poison)
    for nb in (0, 1, 31, 32, 33, 63, 64, 65, 80, 4000):
        for fill in (None, 0x77, 0xFF, 0x00, 0x88, 0x7F):
            for pred in (-32768, 0, 32767):
                for idx in (0, 40, 88):
                    body = g.integers(0, 256, nb, dtype=np.uint8).tobytes() if fill is None else bytes([fill]) * nb
                    rows.append((bytes([(pred >> 8) & 255, pred & 255, idx, 0]) + body, 0))
    for c, name in enumerate(codecs.CODECS[1:], 1):
        for n in (0, 1, 255, 256, 257):
            rows.append((g.integers(0, 256, n * codecs.UNIT[name], dtype=np.uint8).tobytes(), c))
    want = [codecs.reference(p, codecs.CODECS[c]) for p, c in rows]
    n_good = len(rows)
    rows += [(bytes([0, 0, 89, 0]) + bytes(40), 0), (bytes(3), 0), (bytes([0, 0, 0, 0]) + bytes(40), 0),  # index 89; no header; (past stage)
             (bytes(5), 1), (bytes(4), 2), (bytes(8), 7)]  # splits a sample (s16be, s24be); no such codec
    room = [4 * len(w) for w in want] + [4 * 80, 4 * 80, 0, 4 * 2, 4 * 1, 4 * 8]
    offs, front = layout([len(p) for p, _ in rows])
    (_, th), up = layout([front, 4 * codecs.EXPAND_HDR * len(rows)])
    zoffs, zone = layout(room)
    zone += 16  # (a tail the row whose destination leaves the buffer would write over)
    hdr = np.array([[o, len(p), up + z, c] for o, z, (p, c) in zip(offs, zoffs, rows)], dtype=np.int32)
    hdr[n_good + 2, 2] = up + zone - 8  # 80 samples from 8 bytes before the end
    buf, _, (toff,) = pack([p for p, _ in rows], [hdr])
    assert toff == th and buf.numel() == up
    d = torch.full((up + zone,), 0xCD, dtype=torch.uint8, device="cuda")
    d[:up] = buf.cuda()
    before = d[:up].clone()
    most = max(len(w) for w in want)
    assert most == 8000
    check(call_on(d, lib().afx_k_payload_expand, _at(d, 0), d.numel(), _at(d, th), len(rows), most))
    expect = np.full(zone, 0xCD, dtype=np.uint8)
    for z, w in zip(zoffs, want):
        expect[z:z + 4 * len(w)] = w.view(np.uint8)
    got = d.cpu().numpy()
    assert np.array_equal(got[:up], before.cpu().numpy())  # payloads and table are only read
    for i, (z, w) in enumerate(zip(zoffs, want)):
        assert got[up + z:up + z + 4 * len(w)].tobytes() == w.tobytes(), (i, len(w))
    assert np.array_equal(got[up:], expect)  # nothing else is written: the bad rows and every gap keep the poison
    # the saturating contents did reach the clamps
    ends = {(p[4:5], p[2]): w[-1] for (p, c), w in zip(rows[:n_good], want) if c == 0 and len(p) == 4004}
    assert ends[(b"\x77", 88)] == np.float32(32767 / 32768) and ends[(b"\xff", 88)] == np.float32(-1.0)
    # refused on the host, with the entry point's name
    l = lib()
    for args in ((None, 64, _at(d, th), 1, 1), (_at(d, 0), d.numel(), None, 1, 1), (_at(d, 0), d.numel(), _at(d, th), 0, 1),
                 (_at(d, 0), d.numel(), _at(d, th), 65536, 1), (_at(d, 0), d.numel(), _at(d, th), 1, -1),
                 (_at(d, 0), 64, _at(d, th), 1, 17)):
        assert l.afx_k_payload_expand(*args, None) != 0 and b"afx_k_payload_expand" in l.afx_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), got)


def test_decode_takes_the_codecs():
    from afx import codecs
    from afx.ingest import decode
    g = np.random.default_rng(3)
    block = _dvi4(320, g)
    assert torch.equal(decode(block, "dvi4").cpu(), torch.from_numpy(codecs.reference(block, "dvi4")))
    assert decode(bytes(4), "dvi4").shape == (0,)
    for name in codecs.CODECS[1:]:
        raw = g.integers(0, 256, 6 * 101, dtype=np.uint8)
        assert torch.equal(decode(raw, name).cpu(), torch.from_numpy(codecs.reference(raw, name)))
    for bad, name in ((bytes(3), "dvi4"), (bytes([0, 0, 89, 0, 1]), "dvi4"), (bytes(3), "pcm_s16be"), (bytes(4), "pcm_s24be")):
        with pytest.raises(ValueError):
            decode(bad, name)


# ---- PacketScorer ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,codec", [(8000, "dvi4"), (11025, "dvi4"), (48000, "pcm_s24be")])
def test_packet_scorer_in_a_codec_equals_the_native_scorer_fed_the_reference(rate, codec):
    from afx import codecs
    from afx.ingest import PacketScorer
    S = 3
    ta, tb = _tap(S), _tap(S)
    native = "pcm_s16le" if codec == "dvi4" else "pcm_f32le"
    A, B = PacketScorer(ta, rate, codec, max_pending=1), PacketScorer(tb, rate, native, max_pending=1)
    g, rng = np.random.default_rng(rate), random.Random(rate)
    hop_in = H * rate // 16000
    ring = 2 * hop_in  # more input than a slot's pending ring holds
    sizes = [0, 2, rate // 50 // 2 * 2, 2 * ring // 2 * 2 + 6, 2 * 33, 2 * 32, 2 * 31, 640, 1]
    for call in range(12):
        slots = rng.sample(range(S), rng.choice([1, 2, 3]))
        ns = [sizes[(call + 3 * i) % len(sizes)] for i in range(len(slots))]
        if codec == "dvi4":
            pk = [_dvi4(n // 2 * 2, g) for n in ns]
            ref = [_s16le(p) for p in pk]
        else:
            pk = [g.integers(0, 256, 3 * n, dtype=np.uint8).tobytes() for n in ns]
            ref = [codecs.reference(p, codec) for p in pk]
        ra, rb = A.feed(pk, slots), B.feed(ref, slots)
        assert ra.counts.tolist() == rb.counts.tolist()
    assert torch.equal(A.samples_in, B.samples_in) and torch.equal(A.pending, B.pending)
    _same_hops(ta, tb, least=4)
    sa, sb = A.export_slots([0, 1, 2]), B.export_slots([0, 1, 2])
    assert sa.meta == sb.meta and all(torch.equal(sa.tensors[k].cpu(), sb.tensors[k].cpu()) for k in sb.tensors)


# ---- JitterScorer: two codecs per stream, a lossy network ----------------------------------------------------------------
def _network(g):
    """Rows (arrival order) of one 8 kHz stream whose packets alternate mulaw / dvi4: (timestamp, encoding, payload).
    20-ms packets except one DVI4 packet of 30 ms, after which the playout point (hi - 480) falls inside packets; shuffled
    within 60 ms; packet 9 is lost, 14 arrives far too late, 20 (DVI4, 30 ms) arrives when the playout point is inside it,
    some arrive twice, and one extra DVI4 packet overlaps the 40 last samples of an earlier arrival."""
    pk, t = [], 1000
    for k in range(64):
        n = 240 if k == 20 else 160
        enc = "dvi4" if k % 2 == 0 else "mulaw"
        pk.append((t, enc, _dvi4(n, g) if enc == "dvi4" else g.integers(0, 256, n, dtype=np.uint8).tobytes()))
        t += n
    order = list(range(64))
    for a in range(3, 18, 3):
        order[a:a + 3] = order[a:a + 3][::-1]
    order.remove(9)
    order.remove(14)
    order.insert(order.index(30), 14)  # long after the playout point passed it
    order.remove(20)
    order.insert(order.index(22) + 1, 20)  # hi = end of 22: the playout point is 80 samples into packet 20
    calls = []  # one call per arrival; a packet that arrives twice is one call naming the slot twice
    for k in order:
        calls.append([pk[k]] * (2 if k in (5, 26, 41) else 1))
        if k == 36:  # an extra DVI4 packet over [start of 37 - 40, + 160): 40 duplicates, then 120 placed from mid-block
            calls.append([(pk[37][0] - 40, "dvi4", _dvi4(160, g))])
    return calls


def test_jitter_scorer_with_two_codecs_on_a_lossy_network_equals_the_native_one():
    from afx.jitter import JitterScorer
    ta, tb = _tap(2), _tap(2)
    A = JitterScorer(ta, 8000, ("mulaw", "dvi4"), depth=480)
    B = JitterScorer(tb, 8000, ("mulaw", "pcm_s16le"), 480)
    for part in _network(np.random.default_rng(11)):
        slots = [1] * len(part)
        ts = [r[0] for r in part]
        ra = A.feed([r[2] for r in part], slots, ts, encodings=[r[1] for r in part])
        rb = B.feed([_s16le(r[2]) if r[1] == "dvi4" else r[2] for r in part], slots, ts,
                    encodings=["pcm_s16le" if r[1] == "dvi4" else r[1] for r in part])
        assert ra.counts.tolist() == rb.counts.tolist()
    A.flush()
    B.flush()
    sa, sb = A.stats(), B.stats()
    assert all(torch.equal(sa[k], sb[k]) for k in sb)
    assert int(sa["late"][1]) == 160 + 80 and int(sa["duplicate"][1]) == 3 * 160 + 40 + 120 and int(sa["concealed"][1]) == 2 * 160 + 80
    assert torch.equal(A.samples_in, B.samples_in)
    _same_hops(ta, tb, least=4)


# ---- every slot its own rate and codec, fed as RTP ----------------------------------------------------------------------
def _rtp(seq, ts, pt, payload, ssrc):
    return rtp(seq & 0xFFFF, ts & 0xFFFFFFFF, pt=pt, ssrc=ssrc, payload=payload)  # (the callers' counters run past the wrap)


FORMATS = [(8000, "mulaw"), (8000, "dvi4"), (16000, "dvi4"), (44100, "pcm_s16be")]


def test_mixed_jitter_scorer_fed_static_payload_types_equals_the_one_rate_scorers():
    from afx.jitter import JitterScorer, MixedJitterScorer
    S = 3
    tm = _tap(S)
    M = MixedJitterScorer(tm, FORMATS, 60)
    M.reset([1], 16000)
    M.reset([2], 44100)
    one = {0: (8000, ("mulaw", "dvi4")), 1: (16000, "dvi4"), 2: (44100, "pcm_s16be")}
    taps = {s: _tap(S) for s in one}
    J = {s: JitterScorer(taps[s], r, e, 60 * r // 1000) for s, (r, e) in one.items()}
    g = np.random.default_rng(5)
    order = [k for k in range(40) if k not in (6, 21)]
    order[10], order[12], order[30], order[31] = order[12], order[10], order[31], order[30]
    for k in order:
        pt0 = 5 if k % 2 else 0
        d = {0: _rtp(k, (1 << 32) - 800 + 160 * k, pt0, _dvi4(160, g) if pt0 == 5 else g.integers(0, 256, 160, dtype=np.uint8).tobytes(), 0xA),
             1: _rtp(k, 50 + 320 * k, 6, _dvi4(320, g), 0xB),
             2: _rtp(k, 9 + 882 * k, 11, g.integers(0, 256, 2 * 882, dtype=np.uint8).tobytes(), 0xC)}
        named = [2, 0, 1] if k % 2 else [1, 2, 0]
        rm = M.feed_rtp([d[s] for s in named], named)
        for i, s in enumerate(named):
            assert J[s].feed_rtp([d[s]], [s]).counts.tolist() == [int(rm.counts[i])]
    with pytest.raises(ValueError):
        M.feed_rtp([_rtp(99, 0, 5, _dvi4(160, g), 0xB)], [1])  # PT 5 is 8 kHz, slot 1 is at 16 kHz
    with pytest.raises(ValueError):
        M.feed_rtp([_rtp(99, 0, 10, bytes(16), 0xA)], [0])  # stereo L16 is not mapped
    M.flush()
    sm = M.stats()
    for s in one:
        J[s].flush()
        assert len(tm.got[s]) == len(taps[s].got[s]) >= 2 and torch.equal(torch.cat(tm.got[s]), torch.cat(taps[s].got[s]))
        sj = J[s].stats()
        assert all(int(sm[k][s]) == int(sj[k][s]) for k in sj)
    assert sm["concealed"].tolist() == [2 * 160, 2 * 320, 2 * 882]


def test_mixed_packet_scorer_in_codecs_equals_the_one_format_scorers():
    from afx.ingest import MixedPacketScorer, PacketScorer
    S = 4
    tm = _tap(S)
    M = MixedPacketScorer(tm, FORMATS)
    M.reset([0, 1, 2, 3], [0, 1, 2, 3])
    assert [t.encoding for t in M._table] == [2, 0, 0, 0]  # a format in a codec reads the decoded zone
    taps = [_tap(S) for _ in FORMATS]
    P = [PacketScorer(taps[s], r, e) for s, (r, e) in enumerate(FORMATS)]
    g, rng, fed = np.random.default_rng(9), random.Random(9), [0] * S
    for call in range(14):
        n = [rng.choice([0, 80, 160, 1000]), rng.choice([0, 2, 160, 4100]), rng.choice([2, 320, 66, 3000]), rng.choice([1, 882, 9000])]
        pk = [g.integers(0, 256, n[0], dtype=np.uint8).tobytes(), _dvi4(n[1], g), _dvi4(n[2], g),
              g.integers(0, 256, 2 * n[3], dtype=np.uint8).tobytes()]
        named = rng.sample(range(S), rng.choice([2, 3, 4]))
        rm = M.feed([pk[s] for s in named], named)
        for i, s in enumerate(named):
            assert P[s].feed([pk[s]], [s]).counts.tolist() == [int(rm.counts[i])]
            fed[s] += n[s] // 2 * 2 if FORMATS[s][1] == "dvi4" else n[s]
    assert M.samples_in.tolist() == fed
    for s in range(S):  # every slot made the whole hops its samples complete (2, 2, 2 and 3 with these seeds), the same ones
        hops = -(-fed[s] * P[s].L // P[s].M) // H
        assert len(tm.got[s]) == len(taps[s].got[s]) == hops >= 2 and torch.equal(torch.cat(tm.got[s]), torch.cat(taps[s].got[s]))


# ---- one real inner scorer, and a session that changes codec ----------------------------------------------------------------
def test_kv_cached_scores_in_dvi4_equal_pcm_and_a_session_moves_between_them():
    from afx import engine, synth
    from afx.codecs import dvi4_encode
    from afx.jitter import JitterScorer
    from afx.streaming import KVCachedScorer
    sd = synth.model_state_dict("ConformerModel", n_layers=1, n_encoders=1)
    eng = engine.Engine("conformer", n_layers=1, dtype="fp16", conf_blocks=1)
    eng.load_state_dict(sd)
    inner = lambda: KVCachedScorer(eng, sd, 2, window=64000, hop=H)
    A, B, C = (JitterScorer(inner(), 8000, e, depth=480) for e in ("dvi4", "pcm_s16le", "pcm_s16le"))
    g = np.random.default_rng(21)
    state, t, got = [None, None], 0, {"a": [], "b": [], "c": [], "a2": []}
    for k in range(70):
        pk = []
        for s in (0, 1):
            blk, state[s] = dvi4_encode(_speech(160, g, 3000.0), state[s])
            pk.append(blk)
        if k in (17, 44):  # lost, both slots
            t += 160
            continue
        ref = [_s16le(p) for p in pk]
        ra, rb = A.feed(pk, [0, 1], [t, t]), B.feed(ref, [0, 1], [t, t])
        assert ra.counts.tolist() == rb.counts.tolist()
        got["a"].append(ra.scores)
        got["b"].append(rb.scores)
        if k == 30:  # mid-stream, with packets held back in the reorder ring: the dvi4 sessions continue in a pcm scorer
            C.import_slots([0, 1], A.export_slots([0, 1]))
        if k > 30:
            rc = C.feed(ref, [0, 1], [t, t])
            assert rc.counts.tolist() == ra.counts.tolist()
            got["c"].append(rc.scores)
            got["a2"].append(ra.scores)
        t += 160
    a, b = torch.cat(got["a"]), torch.cat(got["b"])
    assert a.numel() >= 8 and torch.equal(a, b)
    assert torch.cat(got["c"]).numel() >= 4 and torch.equal(torch.cat(got["c"]), torch.cat(got["a2"]))
    A.import_slots([0, 1], C.export_slots([0, 1]))  # and back
    assert torch.equal(A.samples_in, C.samples_in)
