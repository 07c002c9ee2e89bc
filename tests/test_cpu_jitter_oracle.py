"""Known answers of the jitter reference itself (oracle/jitter.py).  Every jitter test, CPU and GPU, is held against
``RefSlot``, so its rules are worked out by hand here on streams of a dozen samples: x[i] = i + 1, "repeat" with P = 2 and
F = 3 (the fade weights 1, 2/3, 1/3), depth 0 unless said.  And the seeded traffic of ``Schedule`` is pinned by digest, one
case per payload maker, so that it cannot drift silently: the counters and gap shapes the tests assert depend on it."""
import hashlib

import numpy as np

from oracle.jitter import RefSlot, Schedule, noise_ref, per_packet, voiced_stream, whole_stream
from packet_helpers import bits

W = [np.float32(1.0), np.float32(1.0 - 1 / 3), np.float32(1.0 - 2 / 3)]  # fade[d] = 1 - d / F
X = np.arange(1, 41, dtype=np.float32)


def _slot(mode="repeat", depth=0, **kw):
    return RefSlot(depth, mode, 2, 3, **kw)


def _feed(r, *packets, **kw):
    """One call: its packets [a, b) of X, then the playout."""
    for a, b in packets:
        r.packet(a, X[a:b], **kw)
    r.after_feed()


def _is(r, want):
    return len(r.E) == r.next == len(want) and np.array_equal(bits(r.E), bits(want))


def test_a_gap_longer_than_the_fade_in_repeat_and_in_zero():
    r = _slot()
    _feed(r, (0, 4))
    _feed(r, (9, 12))
    # a = 4: E[4 + d] = fade[d] * E[4 - P + d % P] for d < F, then silence
    assert _is(r, [1, 2, 3, 4, W[0] * 3, W[1] * 4, W[2] * 3, 0, 0, 10, 11, 12])
    assert r.stats == dict(received=7, late=0, duplicate=0, concealed=5, out_of_order=0)
    assert "".join(r.kinds) == "rrrrlllllrrr" and r.spans == [[4, 9]] and r.releases == [[], [[4, 9]]] and r.calls == [1]
    assert (r.next, r.hi, r.gap, r.got) == (12, 12, None, {})
    z = _slot("zero")
    _feed(z, (0, 4))
    _feed(z, (9, 12))
    assert _is(z, [1, 2, 3, 4, 0, 0, 0, 0, 0, 10, 11, 12]) and z.stats == r.stats and z.spans == r.spans


def test_the_playout_point_is_hi_minus_depth():
    r = _slot(depth=3)
    _feed(r, (0, 4))
    assert _is(r, [1]) and (r.next, r.hi, sorted(r.got)) == (1, 4, [1, 2, 3])
    _feed(r, (6, 8))  # hi = 8: [1, 5) is released, the gap that begins at 4 is open
    assert _is(r, [1, 2, 3, 4, 3]) and r.gap == 4 and r.spans == [[4, 5]]
    r.release(r.hi)
    assert _is(r, [1, 2, 3, 4, 3, W[1] * 4, 7, 8]) and r.spans == [[4, 6]] and r.calls == [2] and r.gap is None


def test_a_gap_at_the_origin_repeats_zeros():
    r = _slot()
    _feed(r, (3, 5))  # (source index a - P + d % P < 0: E[< 0] = 0)
    assert _is(r, [0, 0, 0, 4, 5]) and r.stats["concealed"] == 3 and r.spans == [[0, 3]]


def test_two_gaps_closer_than_the_period_in_one_release():
    r = _slot()
    _feed(r, (0, 4))
    _feed(r, (5, 6), (7, 9))  # 4 and 6 are lost: the second gap's source [4, 6) holds the first gap's concealed sample
    assert _is(r, [1, 2, 3, 4, 3, 6, 3, 8, 9]) and r.releases[-1] == [[4, 5], [6, 7]] and r.spans == [[4, 5], [6, 7]]
    assert r.stats["concealed"] == 2 and "".join(r.kinds) == "rrrrlrlrr"


def test_a_gap_released_over_three_calls_is_one_span_and_one_period():
    r = _slot()
    _feed(r, (0, 4))
    r.release(6)  # clock-driven playout, beyond hi
    r.release(8)
    assert (r.next, r.hi) == (8, 8) and r.gap == 4
    _feed(r, (10, 12))
    assert _is(r, [1, 2, 3, 4, 3, W[1] * 4, W[2] * 3, 0, 0, 0, 11, 12])
    assert r.spans == [[4, 10]] and r.calls == [3] and r.releases == [[], [[4, 6]], [[6, 8]], [[8, 10]]] and r.periods == []
    # "pitch_sync": the period is estimated once, where the gap opens.  A history of silence gives the fallback, 10 ms.
    p = RefSlot(0, "pitch_sync", rate=8000, hold=1, fade=2)
    p.packet(0, np.zeros(4, np.float32))
    p.after_feed()
    for upto in (6, 8, 10):
        p.release(upto)
    assert p.periods == [80] and p.p == 80 and p.spans == [[4, 10]] and p.calls == [3] and _is(p, [0] * 10)
    assert (p.Pmin, p.Pmax, p.Wc, p.P0, p.Hd, p.F, p.G) == (20, 120, 160, 80, 1, 2, 3) and p.gain.tolist() == [1, 1, 0.5]
    q = RefSlot(0, "pitch_sync", rate=8000)
    assert (q.Hd, q.F) == (80, 400)  # the scorer's defaults: 10 ms and 50 ms


def test_a_mark_turns_a_loss_into_noise_in_mid_gap_and_a_packet_ends_it():
    r = _slot(noise=3)
    _feed(r, (0, 4))
    r.mark(6, 40)
    _feed(r, (9, 11))
    n = [noise_ref(3, i, 40) for i in (6, 7, 8)]  # (the noise function restated with Python integers)
    assert _is(r, [1, 2, 3, 4, 3, W[1] * 4] + n + [10, 11]) and "".join(r.kinds) == "rrrrllnnnrr" and all(n)
    assert r.stats == dict(received=6, late=0, duplicate=0, concealed=2, out_of_order=0, comfort=3, marks=1, marks_late=0)
    assert (r.level, r.marks, r.spans) == (-1, {}, [[4, 9]])
    _feed(r, (12, 13))  # the packet ended the silence: the next gap is loss again
    assert r.E[11] == W[0] * 10 and r.kinds[11] == "l"
    r.mark(14, 50)
    r.mark(16, 60)
    r.release(18)  # a level update in mid-silence; the silence in force goes on over calls
    r.release(19)  # (13 is loss: its source, a - P = 11, is the concealed sample above)
    assert r.E[13] == W[0] * 10 and np.array_equal(bits(r.E[14:]), bits([noise_ref(3, i, 50 if i < 16 else 60) for i in range(14, 19)]))
    assert r.level == 60 and r.gap == 13 and r.stats["comfort"] == 8


def test_late_and_duplicate_marks():
    r = _slot(noise=3)
    r.mark(0, 40)  # before the session's first packet
    _feed(r, (0, 4))
    r.mark(3, 40)  # below the playout point
    r.mark(6, 40)
    r.mark(6, 41)  # the first arrival wins, the second is not counted
    assert r.marks == {6: 40} and (r.stats["marks"], r.stats["marks_late"]) == (1, 2)
    assert set(r.stats) == {"received", "late", "duplicate", "concealed", "out_of_order", "comfort", "marks", "marks_late"}
    assert set(_slot().stats) == {"received", "late", "duplicate", "concealed", "out_of_order"}


def test_duplicate_partly_late_and_out_of_order_packets():
    r = _slot(depth=4)
    r.packet(0, X[0:4])
    r.packet(2, -X[2:6])  # [2, 4) is held already: the first arrival wins
    r.after_feed()
    assert r.stats == dict(received=6, late=0, duplicate=2, concealed=0, out_of_order=0) and (r.next, r.hi) == (2, 6)
    r.packet(0, X[0:4])  # [0, 2) is below the playout point, [2, 4) is held
    assert (r.stats["late"], r.stats["duplicate"], r.stats["out_of_order"]) == (2, 4, 1)
    r.release(r.hi)
    assert _is(r, [1, 2, 3, 4, -5, -6])
    s = _slot(depth=8)
    s.packet(4, X[4:6])
    s.packet(0, X[0:2])  # a timestamp behind an earlier one
    s.packet(2, X[2:4], by_seq=True)  # (the caller counts by sequence number)
    s.packet(6, X[6:8])
    assert s.stats["out_of_order"] == 1 and s.stats["received"] == 8 and s.max_start == 6


def test_a_whole_packet_taken_at_once_is_the_per_sample_path(monkeypatch):
    """``packet`` takes a packet that is all on time and all new in one step; on a lossy Schedule at 8 kHz (duplicates,
    shuffles, a jump) the slot must come out as when every packet goes sample by sample."""
    out = []
    for fast in (True, False):
        monkeypatch.setattr(RefSlot, "FAST", fast)
        sch, r = Schedule(8000, "pcm_s16le", 7, jump=3000, short=40), RefSlot(480, "repeat", 80, 240)
        while not sch.done():
            for ts, t, raw, x, e in sch.tick():
                r.packet(t, x)
            r.after_feed()
        r.release(r.hi)
        out.append(r)
    a, b = out
    assert np.array_equal(bits(a.E), bits(b.E)) and a.stats == b.stats and a.stats["duplicate"] > 0 and a.stats["concealed"] > 3000
    assert (a.kinds, a.releases, a.spans, a.calls, a.next, a.hi) == (b.kinds, b.releases, b.spans, b.calls, b.next, b.hi)


def _digest(s):
    h = hashlib.sha256(repr((s.ticks, s.origin, sorted(s.lost), s.start)).encode())
    for raw, _ in s.pk:
        h.update(raw)
    return h.hexdigest()[:16]


def test_the_seeded_traffic_is_pinned():
    """The digests were taken from the Schedule classes of the test files this module replaced."""
    assert _digest(Schedule(8000, "mulaw", 9062, jump=2925, short=40, payload=whole_stream)) == "2d4fb3a0c3a99d8c"
    assert _digest(Schedule(8000, ("mulaw", "alaw"), 500, short=40, payload=per_packet(quiet=True))) == "257c4908bcb6954e"
    assert _digest(Schedule(8000, ("mulaw", "alaw"), 6, jump=2924, short=40, payload=per_packet(amp=1.0, div=1))) == "17cded6f98c5b22a"
    assert _digest(Schedule(8000, "mulaw", 9155, jump=3205, short=40, payload=voiced_stream(125))) == "8410b19916751b89"
    s = Schedule(8000, "pcm_s16le", 1, lossy=False)
    assert s.lost == set() and sorted({k for t in s.ticks for k in t}) == list(range(72)) and s.size == [160] * 72
    assert len(s.raw) == 2 * 72 * 160 == 2 * len(s.x) and s.tick()[0][1:2] == (0,)
