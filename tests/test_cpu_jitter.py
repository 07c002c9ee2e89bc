"""The jitter buffer (afx/jitter.py, afx/rtp.py) without a GPU.  The reference for the played-out stream E is
oracle/jitter.py's ``RefSlot``, in plain numpy and per sample: a dict of received samples (first arrival wins), the playout
point, and the concealment recurrence over E itself.  ``JitterScorer``'s plan (the rows of afx_k_jitter_place / _conceal /
_release it would launch) is run by its ``NumpyDevice``, the kernels restated on a numpy ring, and what that releases must equal the reference bit for
bit, with its counters, on random arrival sequences (late, partly late, duplicate, overlapping packets, jumps beyond the
ring).  Also: timestamp unwrapping across 2**32, ``rtp.parse`` on hand-built datagrams, the shape of the launch plan
(disjoint rows, gap order, rounds), refusals that leave a host-only scorer unchanged, the state an export adds and the
cross-refusals, and the new entry points in the header, the library and the ctypes table."""
import ctypes
import os
import random
import re
import struct

import numpy as np
import pytest
import torch

import packet_helpers
from oracle.jitter import BPS, NumpyDevice, RefSlot, decode_ref, rtp as _rtp
from packet_helpers import bits as _bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 4000


@pytest.fixture(scope="module", autouse=True)
def built():
    return packet_helpers.built()


def _host(S=3, rate=8000, encoding="pcm_s16le", depth=160, **kw):
    from afx.jitter import JitterScorer
    from afx.streaming import SlidingWindowScorer
    return JitterScorer(SlidingWindowScorer(None, S, window=16000, hop=H, device="cpu"), rate, encoding, depth, **kw)


def _check(js, dev, refs, origin):
    st = js.stats()
    for s, r in enumerate(refs):
        assert np.array_equal(_bits(dev.out[s]), _bits(r.E)), s
        assert int(js.samples_in[s]) == r.next == dev.N[s] and int(js.buffered[s]) == r.hi - r.next
        assert {k: int(v[s]) for k, v in st.items()} == r.stats, (s, r.stats)
        # the exported intervals are exactly what the reference still holds
        ex = js.export_slots([s])
        iv = [v for v in ex.tensors["jitter_intervals"][0].tolist() if v != [-1, -1]]
        assert sorted(i for a, e in iv for i in range(a, e)) == sorted(r.got)
        assert ex.tensors["jitter_book"][0].tolist()[:4] == [origin[s] if origin[s] is not None else 0, int(origin[s] is not None),
                                                             r.next, r.hi]


@pytest.mark.parametrize("mode,encoding,seed", [("repeat", "pcm_s16le", 1), ("repeat", "mulaw", 2), ("zero", "pcm_f32le", 3),
                                                ("repeat", "pcm_f32le", 4)])
def test_placement_playout_and_concealment_equal_a_per_sample_simulation(mode, encoding, seed):
    rng = random.Random(seed)
    g = np.random.default_rng(seed)
    S, depth, P, F = 3, 120, 50, 130
    js = _host(S=S, encoding=encoding, depth=depth, conceal=mode, period=P, fade=F, ts_bits=None)
    assert js.lookback == (P + F if mode == "repeat" else 0) or js.lookback == js.rs.T - 1
    assert js.J == js.lookback + js.W and js.W >= depth
    dev = NumpyDevice(js)
    refs = [RefSlot(depth, mode, P, F) for _ in range(S)]
    origin = [None] * S
    cursor = [0] * S  # where the "sender" of each slot is (relative index)
    bps = BPS[encoding]
    seen_kinds = set()
    for step in range(140):
        if step == 70:  # a reset mid-way: slot 1 starts over, with another origin
            js.reset([1])
            dev.reset(1)
            refs[1], origin[1], cursor[1] = RefSlot(depth, mode, P, F), None, 0
        rows = [rng.randrange(S) for _ in range(rng.choice([1, 1, 2, 3, 4]))]  # a slot may be named more than once
        packets, stamps = [], []
        plan_ref = []
        for s in rows:
            r = refs[s]
            kind = rng.choice(["next", "next", "next", "skip", "old", "dup", "overlap", "jump", "empty", "straddle"])
            n = rng.choice([1, 7, 40, 80, 80, 160])
            if origin[s] is None:
                origin[s] = rng.randrange(-10 ** 6, 10 ** 9)
                t = 0
            elif kind == "next":
                t = cursor[s]
            elif kind == "skip":  # a lost packet, or several: a gap shorter or longer than P and than F
                t = cursor[s] + rng.choice([5, 30, 80, 200, 400])
            elif kind == "old":  # late, or filling a hole if one is still open
                t = max(0, cursor[s] - rng.choice([100, 200, 300, 600]))
            elif kind == "dup":
                t = max(0, cursor[s] - n)
            elif kind == "overlap":
                t = max(0, cursor[s] - n // 2)
            elif kind == "straddle":  # from below the playout point to beyond it
                t, n = max(0, r.next - 20), 60 + max(0, r.hi - r.next)
            elif kind == "jump":  # further than the ring is long
                t = cursor[s] + js.J + rng.choice([1, 77, 3 * js.J])
            else:
                t, n = cursor[s], 0
            seen_kinds.add(kind)
            if encoding == "pcm_f32le":
                raw = g.standard_normal(n).astype("<f4").tobytes()
            else:
                raw = g.integers(0, 256, n * bps).astype(np.uint8).tobytes()
            packets.append(raw)
            stamps.append(origin[s] + t)
            plan_ref.append((s, t, decode_ref(raw, encoding)))
            cursor[s] = max(cursor[s], t + n)
        before = (js.samples_in.tolist(), js.buffered.tolist(), [v.tolist() for v in js.stats().values()])
        plan, pay = js._plan_feed(packets, rows, stamps if step % 2 else np.array(stamps, dtype=np.int64))
        assert (js.samples_in.tolist(), js.buffered.tolist(), [v.tolist() for v in js.stats().values()]) == before  # planning changes nothing
        dev.run(plan, pay)
        js._commit(plan.book)
        for s, t, vals in plan_ref:
            refs[s].packet(t, vals)
        for s in set(rows):
            refs[s].after_feed()
        if step % 17 == 5:  # clock-driven playout, beyond hi every other time
            s = rng.randrange(S)
            if origin[s] is not None:
                upto = refs[s].next + (50 if step % 2 else depth + 90)
                pl = js._plan([s], mode="advance", upto=upto)
                dev.run(pl, [])
                js._commit(pl.book)
                refs[s].release(upto)
                cursor[s] = max(cursor[s], refs[s].hi)
        if step % 23 == 7:
            sub = rng.sample(range(S), 2)
            pl = js._plan(sub, mode="flush")
            dev.run(pl, [])
            js._commit(pl.book)
            for s in sub:
                refs[s].release(refs[s].hi)
        _check(js, dev, refs, origin)
    assert seen_kinds >= {"next", "skip", "old", "dup", "overlap", "jump", "empty", "straddle"}
    tot = {k: sum(r.stats[k] for r in refs) for k in refs[0].stats}
    assert all(v > 0 for v in tot.values()), tot
    assert "conceal" in dev.launches and dev.launches.count("place") > 100
    if mode == "repeat":  # the gap cases assert on values: some concealed samples are non-zero, and some gaps outlast the fade
        assert any(np.count_nonzero(r.E) > r.stats["received"] // 2 for r in refs)


def test_concealment_values_of_hand_made_gaps():
    """Two gaps closer than P in one release (the second repeats the first's concealed samples), a gap longer than F, and a
    gap at the very start (E[<0] = 0), value by value."""
    P, F = 8, 20
    js = _host(S=1, encoding="pcm_f32le", depth=0, conceal="repeat", period=P, fade=F, ts_bits=None)
    dev = NumpyDevice(js)
    x = np.arange(1, 201, dtype=np.float32)
    fade = (1.0 - np.arange(F) / F).astype(np.float32)

    def feed(t, n, stamps_from=1000):
        plan, pay = js._plan_feed([x[t:t + n].tobytes()], [0], [stamps_from + t])
        dev.run(plan, pay)
        js._commit(plan.book)
        return plan

    feed(0, 10)
    # [10, 14) lost, [14, 17) received, [17, 23) lost, [23, 30) received: with depth 0 both gaps are released by one feed
    p1, pay1 = js._plan_feed([x[14:17].tobytes(), x[23:30].tobytes()], [0, 0], [1014, 1023])
    dev.run(p1, pay1)
    js._commit(p1.book)
    assert [op[0] for op in p1.ops] == ["place", "conceal", "conceal", "release"]
    assert p1.ops[1][1].tolist() == [[0, 10 % js.J, 0, 4]] and p1.ops[2][1].tolist() == [[0, 17 % js.J, 0, 6]]
    E = np.array(dev.out[0], dtype=np.float32)
    want = x[:30].copy()
    want[10:14] = fade[:4] * x[2:6]  # E[a - P + d], a = 10
    want[17:23] = fade[:6] * want[9:15]  # a = 17: the source [9, 17) holds the first gap's concealed samples
    assert np.array_equal(_bits(E), _bits(want)) and want[10] == 3.0 and want[18] == np.float32(0.95) * want[10]
    # a gap of 45 > F + P samples: P-periodic under the fade, then zeros
    feed(75, 5)
    E = np.array(dev.out[0], dtype=np.float32)
    gap = E[30:75]
    assert np.array_equal(_bits(gap[:F]), _bits(fade * np.tile(want[22:30], 3)[:F])) and not gap[F:].any() and gap[:F].all()
    assert np.array_equal(E[75:80], x[75:80]) and int(js.stats()["concealed"][0]) == 4 + 6 + 45
    # a stream that starts with a gap (advance before anything but an empty first packet): E[<0] = 0
    js2 = _host(S=1, encoding="pcm_f32le", depth=0, conceal="repeat", period=P, fade=F)
    dev2 = NumpyDevice(js2)
    plan, pay = js2._plan_feed([b""], [0], [5])
    js2._commit(plan.book)
    pl = js2._plan([0], mode="advance", upto=12)
    dev2.run(pl, [])
    js2._commit(pl.book)
    assert dev2.out[0] == [0.0] * 12 and int(js2.samples_in[0]) == 12 and int(js2.buffered[0]) == 0


def test_a_session_exported_mid_gap_continues_in_another_scorer():
    """The ring columns, the open gap's origin and the intervals travel: a session exported while its playout point stands in
    a gap, moved through a state_dict into another slot of another scorer, plays out what one uninterrupted scorer would."""
    from afx.streaming import StreamState
    P, F, depth = 8, 20, 30
    kw = dict(encoding="pcm_f32le", depth=depth, conceal="repeat", period=P, fade=F, ts_bits=None)
    A, B = _host(S=2, **kw), _host(S=3, max_pending=2, **kw)
    da, db = NumpyDevice(A), NumpyDevice(B)
    ref = RefSlot(depth, "repeat", P, F)
    x = np.arange(1, 301, dtype=np.float32)

    def feed(js, dev, slot, t, n):
        plan, pay = js._plan_feed([x[t:t + n].tobytes()], [slot], [t])
        dev.run(plan, pay)
        js._commit(plan.book)
        ref.packet(t, x[t:t + n])
        ref.after_feed()

    feed(A, da, 0, 0, 50)
    feed(A, da, 0, 95, 5)  # hi = 100: [20, 70) is released, the gap that began at 50 is open and goes on to 95
    assert int(A.samples_in[0]) == 70 == ref.next and ref.gap == 50
    st = A.export_slots([0])
    assert st.tensors["jitter_book"][0].tolist()[:5] == [0, 1, 70, 100, 50]
    assert st.tensors["jitter_intervals"][0].tolist() == [[95, 100]]
    ring = st.tensors["jitter_ring"][0].numpy()  # columns [next - lookback, hi) left-aligned, zeros after
    lb = A.lookback
    assert lb == P + F and np.array_equal(ring[:lb], np.array(ref.E[70 - lb:70], dtype=np.float32)) and not ring[lb:lb + 25].any()
    assert np.array_equal(ring[lb + 25:lb + 30], x[95:100]) and ring.size == lb + depth
    B.import_slots([2], StreamState.from_state_dict(st.to("cpu").state_dict()))
    db.out[2], db.N[2] = list(da.out[0]), da.N[0]
    feed(B, db, 2, 72, 8)  # inside the open gap, ahead of the playout point: placed, not late
    feed(B, db, 2, 100, 60)  # hi = 160: [70, 72) still gap of origin 50, [72, 80) received, [80, 95) a new gap, then received
    assert int(B.samples_in[2]) == 130 == ref.next and int(B.stats()["late"][2]) == 0
    assert np.array_equal(_bits(db.out[2]), _bits(ref.E)) and len(ref.E) == 130
    E = np.array(ref.E, dtype=np.float32)
    fade = (1.0 - np.arange(F) / F).astype(np.float32)
    assert not E[70:72].any() and all(E[50:70])  # d = 20, 21 >= F: silence after twenty faded samples
    assert np.array_equal(E[80:95], fade[:15] * np.tile(x[72:80], 2)[:15]) and np.array_equal(E[95:130], x[95:130])
    assert {k: int(v[2]) for k, v in B.stats().items()} == ref.stats
    # the source went on untouched
    assert int(A.samples_in[0]) == 70 and A.export_slots([0]).tensors["jitter_book"][0].tolist()[:5] == [0, 1, 70, 100, 50]


def test_first_arrival_wins_per_sample():
    js = _host(S=1, encoding="pcm_f32le", depth=100, ts_bits=None)
    dev = NumpyDevice(js)
    a, b = np.full(40, 1.0, dtype=np.float32), np.full(40, 2.0, dtype=np.float32)
    for raw, t in ((a, 0), (a, 60), (b, 30)):  # b overlaps both: only its samples [40, 60) are new
        plan, pay = js._plan_feed([raw.tobytes()], [0], [t])
        dev.run(plan, pay)
        js._commit(plan.book)
    rows = plan.ops[0][1].tolist()
    assert plan.ops[0][0] == "place" and rows == [[0, 40, 20, 40]]  # byte offset 40 = sample 10 of b, 20 samples, at column 40
    pl = js._plan([0], mode="flush")
    dev.run(pl, [])
    assert dev.out[0] == [1.0] * 40 + [2.0] * 20 + [1.0] * 40
    st = {k: int(v[0]) for k, v in js.stats().items()}
    assert st == dict(received=100, late=0, duplicate=20, concealed=0, out_of_order=1)


def test_timestamps_unwrap_across_two_to_the_32():
    js = _host(S=2, encoding="pcm_s16le", depth=320)
    dev = NumpyDevice(js)
    g = np.random.default_rng(5)
    n_pk, size = 40, 80
    x = g.integers(-3000, 3000, n_pk * size).astype("<i2")
    start = (1 << 32) - 11 * size - 3  # the stream crosses 2**32 in its twelfth packet
    order = list(range(n_pk))
    rng = random.Random(5)
    for i in range(0, n_pk, 4):  # reordering within the depth
        blk = order[i:i + 4]
        rng.shuffle(blk)
        order[i:i + 4] = blk
    for k in order:
        t = (start + k * size) % (1 << 32)
        plan, pay = js._plan_feed([x[k * size:(k + 1) * size].tobytes()] * 2, [1, 0], [t, t] if k % 2 else np.array([t, t]))
        dev.run(plan, pay)
        js._commit(plan.book)
    pl = js._plan([0, 1], mode="flush")
    dev.run(pl, [])
    js._commit(pl.book)
    want = x.astype(np.float32) / np.float32(32768)
    for s in (0, 1):
        assert np.array_equal(_bits(dev.out[s]), _bits(want))
    st = js.stats()
    assert st["late"].tolist() == [0, 0] and st["concealed"].tolist() == [0, 0] and st["out_of_order"][0] > 5
    assert js.export_slots([0]).tensors["jitter_book"][0, 0].item() == start
    for bad in ([-1], [1 << 32], [1.5], [True], [0, 1]):
        with pytest.raises(ValueError):
            js._plan_feed([b""], [0], bad)


# ---- RTP -----------------------------------------------------------------------------------------------------------------
def test_rtp_parse_on_hand_built_datagrams():
    from afx import rtp
    pay = bytes(range(1, 21))
    p = rtp.parse(_rtp(65535, 0xFFFFFFF0, pt=8, payload=pay, marker=True))
    assert tuple(p[:5]) == (65535, 0xFFFFFFF0, 8, 0x11223344, True) and bytes(p.payload) == pay
    assert isinstance(p.payload, memoryview)  # a view, not a copy
    p = rtp.parse(bytearray(_rtp(7, 160, payload=pay, csrc=(1, 2, 3))))
    assert (p.seq, p.timestamp, p.payload_type, p.marker) == (7, 160, 0, False) and bytes(p.payload) == pay
    p = rtp.parse(memoryview(_rtp(7, 160, payload=pay, csrc=(9,), ext=bytes(8), pad=4)))
    assert bytes(p.payload) == pay
    assert bytes(rtp.parse(_rtp(1, 2, payload=pay, ext=b"")).payload) == pay  # an extension of zero words
    assert bytes(rtp.parse(_rtp(1, 2, payload=b"", pad=1)).payload) == b""
    assert bytes(rtp.parse(_rtp(1, 2)).payload) == b""
    good = _rtp(1, 2, payload=pay)
    bad = [good[:11], _rtp(1, 2, payload=pay, version=1), _rtp(1, 2, payload=pay, version=3), "text", None,
           _rtp(1, 2, csrc=(1, 2))[:16],  # CSRC list cut short
           _rtp(1, 2, ext=bytes(8))[:18],  # extension cut short
           struct.pack("!BBHII", 0x90, 0, 1, 2, 3) + b"\x00\x00",  # extension header cut short
           struct.pack("!BBHII", 0xA0, 0, 1, 2, 3) + bytes([1, 2, 9]),  # padding count beyond the payload
           struct.pack("!BBHII", 0xA0, 0, 1, 2, 3) + bytes([1, 2, 0]),  # padding count zero
           struct.pack("!BBHII", 0xA0, 0, 1, 2, 3)]  # padding bit without a byte to count
    for d in bad:
        with pytest.raises(ValueError):
            rtp.parse(d)


def test_feed_rtp_checks_payload_type_and_ssrc_and_counts_by_sequence_number():
    js = _host(S=2, encoding="mulaw", depth=160)
    pay = bytes(80)
    plan_before = js.export_slots([0, 1])
    for dgrams, kw in (([_rtp(1, 0, pt=8, payload=pay)], {}), ([_rtp(1, 0, pt=96, payload=pay)], {}),
                       ([_rtp(1, 0, pt=96, payload=pay)], dict(payload_types={96: "alaw"})),
                       ([_rtp(1, 0, payload=pay), _rtp(2, 80, payload=pay, ssrc=5)], {}), ([_rtp(1, 0, payload=pay)[:8]], {})):
        with pytest.raises(ValueError):
            js.feed_rtp(dgrams, [0] * len(dgrams), **kw)
    assert all(torch.equal(plan_before.tensors[k], js.export_slots([0, 1]).tensors[k]) for k in plan_before.tensors)
    # an empty payload plans no launch, so this runs on a host-only scorer: the SSRC is set, sequence numbers are counted
    empty = lambda seq, ts, **kw: _rtp(seq, ts, payload=b"", **kw)
    js.feed_rtp([empty(65534, 0), empty(65535, 80), empty(1, 240), empty(0, 160)], [0, 0, 0, 0])
    assert int(js.stats()["out_of_order"][0]) == 1  # 0 after 1, across the 16-bit wrap
    assert js.export_slots([0]).tensors["jitter_book"][0].tolist()[6:] == [1, 0x11223344]
    with pytest.raises(ValueError):
        js.feed_rtp([empty(2, 320, ssrc=7)], [0])
    js.feed_rtp([empty(2, 320, ssrc=7)], [1])  # another slot, another session
    js.reset([0])
    js.feed_rtp([empty(9, 0, ssrc=7)], [0])  # after a reset the next datagram sets the SSRC
    dyn = _host(S=1, encoding="pcm_s16le", depth=0)
    with pytest.raises(ValueError):
        dyn.feed_rtp([empty(1, 0, pt=97)], [0])
    dyn.feed_rtp([empty(1, 0, pt=97)], [0], payload_types={97: "pcm_s16le"})


# ---- the launch plan -----------------------------------------------------------------------------------------------------
def test_launch_plan_rounds_for_a_packet_longer_than_the_ring_and_the_common_case_is_one_round():
    js = _host(S=4, rate=8000, encoding="mulaw", depth=480, ts_bits=None)
    dev = NumpyDevice(js)
    assert js.period == 80 and js.fade_len == 240  # the defaults: 10 ms and 3 P
    assert js.W == 480 + 2000 + 1 and js.J == js.W + max(js.rs.T - 1, 320)
    g = np.random.default_rng(0)
    pk = lambda n: g.integers(0, 256, n).astype(np.uint8).tobytes()
    # the common case: every slot continues at its hi -> one place, one release, no per-slot work, pops when a hop completes
    t = 0
    for k in range(30):
        plan, pay = js._plan_feed([pk(160)] * 4, [3, 1, 0, 2], [t] * 4)
        dev.run(plan, pay)
        js._commit(plan.book)
        kinds = [op[0] for op in plan.ops]
        assert kinds[0] == "place" and kinds.count("place") == 1 and kinds.count("release") <= 1 and "conceal" not in kinds
        assert plan.ops[0][1][:, 0].tolist() == [3, 1, 0, 2]
        t += 160
        assert not js._b.holes and not js._b.holey.any()
    assert js.samples_in.tolist() == [30 * 160 - 480] * 4 and "pop" in dev.launches
    # one packet of 3.5 rings for slot 2 (and an ordinary one for slot 0): rounds of at most W samples, in order
    n = int(3.5 * js.J)
    big = pk(n)
    plan, pay = js._plan_feed([big, pk(160)], [2, 0], [t, t])
    places = [op for op in plan.ops if op[0] == "place"]
    assert len(places) >= 4 and all(op[2] <= js.W for op in places)
    got = [r for op in places for r in op[1].tolist() if r[0] == 2]
    assert sum(r[2] for r in got) == n and [r[1] for r in got] == (np.cumsum([0] + [r[2] for r in got[:-1]])).tolist()
    dev.run(plan, pay)
    js._commit(plan.book)
    assert int(js.samples_in[2]) == t + n - 480 and plan.counts.tolist() == [(-(-(t + n - 480) * 2) // H) - (30 * 160 - 480) * 2 // H, 0]
    assert np.array_equal(_bits(dev.out[2][t:]), _bits(decode_ref(big, "mulaw")[:n - 480]))
    # buffered feeds: refused when the pending ring would overflow, and nothing has changed then
    before = js.export_slots([0, 1, 2, 3])
    with pytest.raises(ValueError):
        js._plan_feed([pk(4 * H)], [1], [t], score=False)
    after = js.export_slots([0, 1, 2, 3])
    assert all(torch.equal(before.tensors[k], after.tensors[k]) for k in before.tensors)


def test_refusals_leave_a_host_scorer_unchanged():
    from afx._lib import AfxError
    from afx.jitter import JitterScorer
    from afx.streaming import SlidingWindowScorer
    sc = SlidingWindowScorer(None, 2, window=16000, hop=H, device="cpu")
    for kw in (dict(depth=-1), dict(depth=1.5), dict(depth=True), dict(conceal="pitch"), dict(period=0), dict(fade=-1),
               dict(max_pending=0), dict(ts_bits=3), dict(encoding="g722"), dict(input_rate=7999)):
        args = dict(dict(input_rate=8000, encoding="mulaw", depth=480), **kw)
        with pytest.raises(ValueError):
            JitterScorer(sc, **args)
    js = _host(S=2, encoding="pcm_s16le", depth=160)
    assert js.S == 2 and js.device.type == "cpu" and js.delay == 20 and js.hop == H
    pk = np.zeros(80, dtype=np.int16)
    plan, pay = js._plan_feed([pk.tobytes()], [1], [77])  # give slot 1 a session without a GPU: a packet inside the depth
    assert [op[0] for op in plan.ops] == ["place"]
    js._commit(plan.book)

    def snap():
        e = js.export_slots([0, 1])
        return [js.pending, js.samples_in, js.buffered, js.samples_seen] + list(js.stats().values()) + [e.tensors[k] for k in sorted(e.tensors)]

    before = snap()
    bad = [(([pk], [0, 1], [0, 0]), {}), (([pk, pk], [0], [0]), {}), (([pk, pk], [0, 2], [0, 0]), {}), (([pk, pk], [0, 1], [0]), {}),
           (([pk, b"abc"], [0, 1], [0, 0]), {}), (([pk, pk.astype(np.float32)], [0, 1], [0, 0]), {}), ((pk.tobytes(), [0], [0]), {}),
           (([pk, pk], [True, True], [0, 0]), {}), (([pk, pk], [0.0, 1.0], [0, 0]), {}), (([pk], [0], [0.5]), {}),
           (([pk], [0], [1 << 32]), {}), (([pk], [0], ["0"]), {}),
           (([np.zeros(4 * H // 2 + 200, dtype=np.int16)], [0], [0]), dict(score=False))]
    for args, kw in bad:
        with pytest.raises(ValueError):
            js.feed(*args, **kw)
        assert all(torch.equal(a, b) for a, b in zip(before, snap()))
    for call in (lambda: js.drain([2]), lambda: js.flush([0, 0]), lambda: js.advance([0], 5),  # (slot 0 has no origin yet)
                 lambda: js.advance([1], -1), lambda: js.advance([1], [1, 2]), lambda: js.advance([1], 1.5)):
        with pytest.raises(ValueError):
            call()
        assert all(torch.equal(a, b) for a, b in zip(before, snap()))
    for call in (lambda: js.feed([pk, pk], [0, 1], [0, 157]), lambda: js.flush([1]), lambda: js.advance([1], 10)):
        with pytest.raises(AfxError):  # valid, but there is no GPU behind this scorer: nothing changes either
            call()
        assert all(torch.equal(a, b) for a, b in zip(before, snap()))
    res = js.feed([b"", bytearray()], [1, 0], [500, 0])  # empty packets are legal and complete nothing
    assert res.counts.tolist() == [0, 0] and res.scores.numel() == 0
    assert js.drain().counts.tolist() == [0, 0] and js.advance([1], 0).counts.tolist() == [0]
    assert js.feed([], [], []).counts.tolist() == [] and js.feed_rtp([], []).counts.tolist() == []  # a tick without a packet
    js.reset([1])
    assert js.buffered.tolist() == [0, 0] and js.samples_in.tolist() == [0, 0] and not any(v.any() for v in js.stats().values())


def test_state_keys_meta_and_cross_refusals():
    from afx.ingest import PacketScorer
    from afx.jitter import JITTER_FORMAT
    from afx.streaming import ResamplingScorer, SlidingWindowScorer, StreamState
    js = _host(S=2, rate=48000, depth=2880, max_pending=3)
    g = np.random.default_rng(1)
    for s, t, n in ((0, 100, 960), (0, 100 + 1920, 960), (1, 7, 480)):  # slot 0 holds a hole inside its depth
        plan, pay = js._plan_feed([g.integers(-9, 9, n).astype("<i2").tobytes()], [s], [t])
        assert all(op[0] == "place" for op in plan.ops)
        js._commit(plan.book)
    st = js.export_slots([1, 0])
    assert set(st.tensors) == {"samples", "jitter_pending", "jitter_fill", "jitter_ring", "jitter_book", "jitter_stats",
                               "jitter_intervals"}
    assert tuple(st.tensors["jitter_pending"].shape) == (2, 3 * H)
    assert tuple(st.tensors["jitter_ring"].shape) == (2, js.lookback + 2880) and js.lookback == 480 + 3 * 480
    assert st.tensors["jitter_intervals"].tolist() == [[[0, 480], [-1, -1]], [[0, 960], [1920, 2880]]]
    assert st.tensors["jitter_book"].tolist() == [[7, 1, 0, 480, -1, 0, -1, -1], [100, 1, 0, 2880, -1, 1920, -1, -1]]
    assert st.tensors["jitter_stats"].tolist() == [[480, 0, 0, 0, 0], [1920, 0, 0, 0, 0]]
    assert all(st.tensors[k].dtype == torch.int64 for k in ("jitter_fill", "jitter_book", "jitter_stats", "jitter_intervals"))
    want = dict(input_rate=48000, resampler="kaiser5-hl10", jitter=JITTER_FORMAT, jitter_depth=2880, jitter_conceal="repeat",
                jitter_period=480, jitter_fade=1440)
    assert {k: st.meta[k] for k in want} == want and js.state_meta() == st.meta and "encoding" not in st.meta
    st2 = StreamState.from_state_dict(st.to("cpu").state_dict())
    other = _host(S=3, rate=48000, encoding="alaw", depth=2880, max_pending=1)  # any encoding, any S, any max_pending that fits
    other.import_slots([2, 0], st2)
    back = other.export_slots([2, 0])
    assert all(torch.equal(back.tensors[k], st.tensors[k]) for k in st.tensors if k != "jitter_pending")
    assert other.buffered.tolist() == [2880, 0, 480] and other.stats()["received"].tolist() == [1920, 0, 480]
    bare = SlidingWindowScorer(None, 2, window=16000, hop=H, device="cpu")
    wrapped = ResamplingScorer(SlidingWindowScorer(None, 2, window=16000, hop=H, device="cpu"), 48000)
    packet = PacketScorer(SlidingWindowScorer(None, 2, window=16000, hop=H, device="cpu"), 48000, "pcm_s16le", 3)
    for dst in (bare, wrapped, packet):
        with pytest.raises(ValueError):
            dst.import_slots([0, 1], st)
    keep = js.export_slots([0, 1])
    foreign = [bare.export_slots([0, 1]), wrapped.export_slots([0, 1]), packet.export_slots([0, 1]), st.tensors, None,
               _host(S=2, rate=24000, depth=2880).export_slots([0, 1]), _host(S=2, rate=48000, depth=2881).export_slots([0, 1]),
               _host(S=2, rate=48000, depth=2880, conceal="zero").export_slots([0, 1]),
               _host(S=2, rate=48000, depth=2880, period=481).export_slots([0, 1]),
               _host(S=2, rate=48000, depth=2880, fade=1441).export_slots([0, 1])]
    for f in foreign:
        with pytest.raises(ValueError):
            js.import_slots([0, 1], f)
    for key, val in (("resampler", "other"), ("jitter", JITTER_FORMAT + 1), ("hop", 2000)):
        with pytest.raises(ValueError):
            js.import_slots([0, 1], StreamState(dict(st.meta, **{key: val}), st.seen, st.tensors))
    with pytest.raises(ValueError):
        js.import_slots([0], st)  # two sessions for one slot

    def edited(key, fn):
        t = {k: v.clone() for k, v in st.tensors.items()}
        fn(t[key])
        return StreamState(st.meta, st.seen, t)

    def set_(r, c, v):
        return lambda t: t[r].__setitem__(c, v)

    contradictions = [edited("jitter_book", set_(0, 2, 5)),  # next = 5 without any sample scored or pending
                      edited("jitter_book", set_(0, 3, 479)),  # hi below the last interval's end
                      edited("jitter_book", set_(1, 3, 2881)),  # more held back than the depth
                      edited("jitter_book", set_(0, 4, 3)),  # an open gap at or beyond the playout point
                      edited("jitter_book", set_(0, 1, 2)), edited("jitter_stats", set_(0, 0, 479)),  # fewer received than held
                      edited("jitter_stats", set_(1, 3, 1)),  # concealed samples beyond the playout point
                      edited("jitter_stats", set_(1, 1, -1)), edited("jitter_fill", lambda t: t.__setitem__(0, 1)),
                      edited("jitter_intervals", lambda t: t[1, 1].__setitem__(0, 900)),  # overlapping intervals
                      edited("jitter_intervals", lambda t: t[0, 0].__setitem__(0, -3))]
    for bad in contradictions:
        with pytest.raises(ValueError):
            js.import_slots([0, 1], bad)
    now = js.export_slots([0, 1])
    assert all(torch.equal(keep.tensors[k], now.tensors[k]) for k in keep.tensors)
    big = _host(S=1, rate=48000, depth=2880, max_pending=3).export_slots([0])
    big.tensors["jitter_fill"] = torch.tensor([2 * H + 1])
    big.tensors["jitter_book"][0, 1:4] = torch.tensor([1, 3 * (2 * H + 1), 3 * (2 * H + 1)])
    with pytest.raises(ValueError):
        _host(S=1, rate=48000, depth=2880, max_pending=2).import_slots([0], big)
    js.import_slots([1], big)
    assert js.pending.tolist() == [0, 2 * H + 1] and js.samples_in.tolist() == [0, 3 * (2 * H + 1)]


def test_jitter_entry_points_are_in_header_library_and_ctypes_table(built):
    _lib = built
    src = open(os.path.join(ROOT, "include", "afx.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("afx_k_jitter_place", "afx_k_jitter_conceal", "afx_k_jitter_release"):
        assert re.search(r"\b%s\s*\(" % name, src) and hasattr(lib, name) and name in _lib.SIGNATURES
    l = _lib.lib()
    # refused on the host: nothing is launched (there is no GPU here to launch on)
    assert l.afx_k_jitter_place(None, 0, None, 1, 1, 0, None, 1, 1, None) != 0 and b"jitter_place" in l.afx_last_error()
    assert l.afx_k_jitter_conceal(None, 1, 1, None, 1, 1, None, 1, 1, 1, None) != 0 and b"jitter_conceal" in l.afx_last_error()
    assert l.afx_k_jitter_release(None, 1, 1, None, 1, 1, None, 1, 1, 1, None, 1, None) != 0 and b"jitter_release" in l.afx_last_error()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert l.afx_k_jitter_place(p, 64, p, 1, 17, 0, p, 1, 16, None) != 0 and b"fit" in l.afx_last_error()  # max_n > J
    assert l.afx_k_jitter_place(p, 64, p, 1, 1, 4, p, 1, 16, None) != 0 and b"encoding" in l.afx_last_error()
    assert l.afx_k_jitter_conceal(p, 1, 16, p, 1, 9, p, 8, 4, 1, None) != 0 and b"fit" in l.afx_last_error()  # max_n + P > J
    assert l.afx_k_jitter_conceal(p, 1, 16, p, 1, 1, p, 8, 4, 2, None) != 0 and b"mode" in l.afx_last_error()
    assert l.afx_k_jitter_conceal(p, 1, 16, p, 1, 1, None, 8, 4, 1, None) != 0 and b"fade" in l.afx_last_error()
    assert l.afx_k_jitter_release(p, 1, 16, p, 1, 9, p, 1, 1, 1, p, 8, None) != 0 and b"fit" in l.afx_last_error()  # max_out > ring_len
    assert l.afx_k_jitter_release(p, 1, 16, p, 1, 1, None, 2, 1, 1, p, 8, None) != 0 and b"identity" in l.afx_last_error()
    assert l.afx_k_jitter_release(p, 1, 16, p, 1, 1, p, 1, 2, 18, p, 8, None) != 0 and b"history" in l.afx_last_error()
    assert l.afx_k_jitter_release(p, 1, 16, p, 0, 1, p, 1, 2, 8, p, 8, None) != 0 and b"rows" in l.afx_last_error()
