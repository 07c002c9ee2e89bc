"""Silence suppression and comfort noise in the jitter buffer (afx/jitter.py ``ComfortNoise``, ``silence``, ``feed_rtp`` with
RFC 3389 payloads) without a GPU.  The reference for the played-out stream E is oracle/jitter.py's ``RefSlot``, per sample: a dict of
received samples, a dict of silence marks, the playout point, and for every released index either its received value, comfort
noise at the level of the latest mark of its run of missing samples, or the loss concealment of the contract.  The planner's
launches (place, noise, conceal, release) are run by its ``NumpyDevice``, the kernels restated on the scorer's own ring, and
what that releases must equal the reference bit for bit, with its counters.  Also: known answers and statistics of the noise
function, hand-made gaps, "no marks, no change", ``feed_rtp``, sessions moved mid-silence, the mixed-rate scorer against
the one-rate scorer, and the new entry points in the header, the library and the ctypes table."""
import ctypes
import os
import random
import re

import numpy as np
import pytest
import torch

import packet_helpers
from oracle.jitter import NumpyDevice as _Device, RefSlot, dtx_events, k_ref, noise_ref, rtp as _rtp
from packet_helpers import bits as _bits, go as _go, inner as _inner

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 4000


@pytest.fixture(scope="module", autouse=True)
def built():
    return packet_helpers.built()


def test_known_answers_of_the_noise_function():
    from afx.jitter import ComfortNoise
    assert ComfortNoise().seed == 0
    assert ComfortNoise(0).ints(0, 4).tolist() == [0, 130277, 325842, 1018909]
    assert ComfortNoise(1).ints(0, 4).tolist() == [6850960, -6336426, 4441393, -866810]
    assert [k_ref(1, i) for i in range(4)] == [6850960, -6336426, 4441393, -866810]
    cn = ComfortNoise(12345)
    assert cn.amp.dtype == np.float32 and cn.amp.shape == (128,)
    for l in (0, 60, 127):
        assert cn.amp[l] == np.float32(np.sqrt(3.0) * 10.0 ** (-l / 20.0) / 2.0 ** 23)
    i0 = (1 << 32) - 2  # crosses into the high half of the index
    got = cn.samples(i0, 6, 60)
    assert got.dtype == np.float32 and np.array_equal(_bits(got), _bits([noise_ref(12345, i0 + k, 60) for k in range(6)]))
    assert np.array_equal(cn.ints(i0, 6), np.array([k_ref(12345, i0 + k) for k in range(6)]))
    assert not np.array_equal(cn.samples(i0, 6, 60)[:2], cn.samples(i0 + (1 << 32), 6, 60)[:2])  # hi32 matters
    assert not np.array_equal(cn.ints(2, 4), cn.ints(2 + (1 << 32), 4))
    k = cn.ints(0, 8000)
    assert k.min() >= -(1 << 23) and k.max() < 1 << 23 and np.array_equal(k.astype(np.float32).astype(np.int64), k)
    for bad in (-1, 1 << 32, 1.5, True, "0", None):
        with pytest.raises(ValueError):
            ComfortNoise(bad)
    for bad in (-1, 128, 1.0, True):
        with pytest.raises(ValueError):
            cn.samples(0, 4, bad)


def test_noise_statistics_on_one_fixed_input():
    """Seed 12345, indices 0..7999, level 60: uniform white noise of RMS 1e-3.  The RMS estimator's relative sigma at N = 8000
    uniform samples is 0.5 %, so 3 % is 6 sigma; an autocorrelation estimate's sigma is 1/sqrt(8000) = 0.011, so 0.05 is
    4.5 sigma."""
    from afx.jitter import ComfortNoise
    x = ComfortNoise(12345).samples(0, 8000, 60).astype(np.float64)
    rms = np.sqrt(np.mean(x * x))
    assert abs(rms / 1e-3 - 1) < 0.03, rms
    assert abs(x.mean()) < 5 * 1e-3 / np.sqrt(8000)
    for lag in (1, 2, 3, 80, 160):
        r = np.sum(x[lag:] * x[:-lag]) / np.sum(x * x)
        assert abs(r) < 0.05, (lag, r)
    assert np.abs(x).max() <= np.sqrt(3.0) * 1e-3 * (1 + 1e-6)  # uniform: bounded by sqrt(3) RMS, nothing clipped


def NumpyDevice(js):
    return _Device(js, count_pops=True)  # (the inner session counts the hop it would have been pushed)


def _host(S=3, rate=8000, encoding="pcm_f32le", depth=160, seed=7, **kw):
    from afx.jitter import ComfortNoise, JitterScorer
    cn = None if seed is None else ComfortNoise(seed)
    return JitterScorer(_inner(S), rate, encoding, depth, comfort_noise=cn, **kw)


def _stats(js, s):
    return {k: int(v[s]) for k, v in js.stats().items()}


@pytest.mark.parametrize("rate", [8000, 16000])
@pytest.mark.parametrize("mode", ["repeat", "zero"])
def test_played_out_stream_with_marks_equals_a_per_sample_simulation(mode, rate):
    S, depth, seed = 2, 3 * (rate // 50), 99
    P, F = (rate // 100, 3 * (rate // 100)) if mode == "repeat" else (0, 0)
    js = _host(S=S, rate=rate, depth=depth, conceal=mode, seed=seed)
    dev = NumpyDevice(js)
    refs = [RefSlot(depth, mode, P, F, noise=seed) for _ in range(S)]
    origin = [(1 << 32) - 5 * (rate // 50) - 3, 123456]  # slot 0's timestamps wrap in its sixth packet
    ev = [dtx_events(rate, 1000 * rate // 8000 + 17 * s + (5 if mode == "zero" else 0)) for s in range(S)]
    at = [0] * S
    rng = random.Random(rate + len(mode))
    silent = [False] * S  # the last event taken from the slot's traffic was a CN
    pieces = 0
    step = 0
    while any(at[s] < len(ev[s]) for s in range(S)):
        step += 1
        rows = []
        for s in range(S):
            if at[s] < len(ev[s]) and rng.random() < 0.75:
                m = rng.randint(1, 3)
                rows += [(s,) + e for e in ev[s][at[s]:at[s] + m]]
                at[s] += m
        if not rows:
            continue
        order = [r[0] for r in rows]
        rng.shuffle(order)  # the slots' rows interleaved, each slot's own rows in their order of arrival
        its = {s: iter([r for r in rows if r[0] == s]) for s in range(S)}
        rows = [next(its[s]) for s in order]
        marks =[(s, (origin[s] + t) % (1 << 32), l) for s, kind, t, l in rows if kind == "cn"]
        audio = [(s, (origin[s] + t) % (1 << 32), t, x) for s, kind, t, x in rows if kind == "pkt"]
        for s, kind, t, v in rows:  # the marks of a call are registered before its audio
            if kind == "cn":
                refs[s].mark(t, v)
        mk = tuple(list(c) for c in zip(*marks)) if marks else None
        if mk and step % 2:  # every other time through the public call, then a feed without marks
            js.silence(*mk)
            mk = None
        plan, pay = js._plan_feed([a[3].tobytes() for a in audio], [a[0] for a in audio], [a[1] for a in audio], marks=mk)
        _go(js, dev, plan, pay)
        named = []
        for s, ts, t, x in audio:
            refs[s].packet(t, x)
            named += [s] if s not in named else []
        for s in named:
            refs[s].after_feed()
        for s in range(S):
            mine = [r for r in rows if r[0] == s]
            if mine:
                silent[s] = mine[-1][1] == "cn"
        for s in range(S):  # clock-driven playout through a silence, in several pieces, one of them longer than the ring
            if silent[s] and refs[s].started and rng.random() < 0.5:
                for piece in (37, rate // 25, js.J + 50) if pieces % 3 == 0 else (rate // 50,):
                    upto = refs[s].hi + piece - depth // 2
                    _go(js, dev, js._plan([s], mode="advance", upto=upto))
                    refs[s].release(max(refs[s].next, upto))
                pieces += 1
        if step % 19 == 7:
            _go(js, dev, js._plan(list(range(S)), mode="flush"))
            for r in refs:
                r.release(r.hi)
        for s, r in enumerate(refs):
            assert np.array_equal(_bits(dev.out[s]), _bits(r.E)), (step, s)
            assert _stats(js, s) == r.stats, (step, s, _stats(js, s), r.stats)
            assert int(js.samples_in[s]) == r.next == dev.N[s] and int(js.buffered[s]) == r.hi - r.next
            ex = js.export_slots([s])
            got = [v for v in ex.tensors["jitter_cn_marks"][0].tolist() if v != [-1, -1]]
            assert got == sorted([t, l] for t, l in r.marks.items())
            assert int(ex.tensors["jitter_cn_open"][0]) == (r.level if r.gap is not None else -1)
    _go(js, dev, js._plan(list(range(S)), mode="flush"))
    tot = {k: 0 for k in refs[0].stats}
    for s, r in enumerate(refs):
        r.release(r.hi)
        assert np.array_equal(_bits(dev.out[s]), _bits(r.E)) and _stats(js, s) == r.stats
        for k in tot:
            tot[k] += r.stats[k]
    kinds = "|".join("".join(r.kinds) for r in refs)
    for pat in ("rl", "ln", "rn", "nr"):  # loss after speech, loss then noise in one run, noise at a spurt's end, speech after noise
        assert pat in kinds, pat
    assert all(v > 0 for k, v in tot.items() if k != "duplicate"), tot
    assert pieces >= 3 and dev.noise_rows > 20 and "conceal" in dev.launches


# ---- hand-made gaps ---------------------------------------------------------------------------------------------------------------
def _hand(P=8, F=20, depth=0, seed=3, **kw):
    js = _host(S=1, depth=depth, conceal="repeat", period=P, fade=F, ts_bits=None, seed=seed, **kw)
    return js, NumpyDevice(js)


def _feed(js, dev, x, t, n, marks=None):
    plan, pay = js._plan_feed([x[t:t + n].tobytes()], [0], [t], marks=marks)
    return _go(js, dev, plan, pay)


def test_a_mark_inside_a_gap_splits_it_into_faded_repetition_and_noise():
    from afx.jitter import ComfortNoise
    P, F = 8, 20
    js, dev = _hand(P, F)
    cn = ComfortNoise(3)
    x = np.arange(1, 201, dtype=np.float32)
    fade = (1.0 - np.arange(F) / F).astype(np.float32)
    _feed(js, dev, x, 0, 10)
    js.silence([0], [16], [40])  # the last packet of the spurt, [10, 16), is lost; silence from 16 on
    p = _feed(js, dev, x, 60, 10)
    assert [op[0] for op in p.ops] == ["place", "noise", "conceal", "release"]
    assert p.ops[1][1].tolist() == [[0, 16 % js.J, 44, 16, 0, 40]] and p.ops[2][1].tolist() == [[0, 10 % js.J, 0, 6]]
    E = np.array(dev.out[0], dtype=np.float32)
    assert np.array_equal(E[10:16], fade[:6] * x[2:8])  # [g, t): loss, d = i - g
    assert np.array_equal(_bits(E[16:60]), _bits(cn.samples(16, 44, 40)))  # [t, b): noise whatever d is (44 > F)
    assert np.array_equal(E[60:70], x[60:70])
    assert _stats(js, 0) == dict(received=20, late=0, duplicate=0, concealed=6, out_of_order=0, comfort=44, marks=1, marks_late=0)
    # a loss gap directly after a received packet that followed noise: its source [a - P, a) = 2 noise samples + 6 received
    js2, dev2 = _hand(P, F)
    _feed(js2, dev2, x, 0, 10)
    _feed(js2, dev2, x, 30, 6, marks=([0], [10], [50]))
    _feed(js2, dev2, x, 50, 5)
    E = np.array(dev2.out[0], dtype=np.float32)
    src = np.concatenate([cn.samples(28, 2, 50), x[30:36]])
    assert np.array_equal(_bits(E[10:30]), _bits(cn.samples(10, 20, 50)))
    assert np.array_equal(_bits(E[36:50]), _bits(fade[:14] * np.tile(src, 2)[:14])) and E[36] == cn.samples(28, 1, 50)[0]
    # the same gap and its noise source released in ONE call: the noise launch goes before the conceal rank that reads it
    js3, dev3 = _hand(P, F, depth=100)
    _feed(js3, dev3, x, 0, 10)
    _feed(js3, dev3, x, 30, 6, marks=([0], [10], [50]))
    _feed(js3, dev3, x, 50, 5)
    p = _go(js3, dev3, js3._plan([0], mode="flush"))
    assert [op[0] for op in p.ops] == ["noise", "conceal", "release"]
    assert np.array_equal(_bits(dev3.out[0]), _bits(E))


def test_a_mark_update_in_mid_gap_and_a_mark_inside_a_received_interval():
    from afx.jitter import ComfortNoise
    js, dev = _hand()
    cn = ComfortNoise(3)
    x = np.arange(1, 201, dtype=np.float32)
    _feed(js, dev, x, 0, 10)
    js.silence([0, 0, 0, 0], [10, 40, 40, 95], [30, 70, 71, 20])  # an update at 40 (its duplicate loses); 95 is inside a packet
    assert _stats(js, 0)["marks"] == 3
    p = _feed(js, dev, x, 90, 10)
    assert [r[1:] for r in p.ops[1][1].tolist()] == [[10 % js.J, 30, 10, 0, 30], [40 % js.J, 50, 40, 0, 70]]
    assert "conceal" not in [op[0] for op in p.ops]
    E = np.array(dev.out[0], dtype=np.float32)
    assert np.array_equal(_bits(E[10:40]), _bits(cn.samples(10, 30, 30))) and np.array_equal(_bits(E[40:90]), _bits(cn.samples(40, 50, 70)))
    assert np.array_equal(E[90:100], x[90:100])  # received samples are never modified
    # the mark at 95 was inside a received interval: the next gap is loss, not noise
    _feed(js, dev, x, 110, 5)
    E = np.array(dev.out[0], dtype=np.float32)
    fade = (1.0 - np.arange(20) / 20).astype(np.float32)
    assert np.array_equal(E[100:110], fade[:10] * np.tile(x[92:100], 2)[:10])
    assert _stats(js, 0) == dict(received=25, late=0, duplicate=0, concealed=10, out_of_order=0, comfort=80, marks=3, marks_late=0)
    assert not js._b.marks
    # a mark below the playout point, and one for a slot without a session, are dropped and counted; the released stream stays
    js.silence([0], [50], [10])
    other = _host(S=2, seed=3)
    other.silence([1], [0], [10])
    assert _stats(js, 0)["marks_late"] == 1 and _stats(other, 1)["marks_late"] == 1 and not other._b.marks
    # a mark at t > next for a gap that is open: noise from its t on, in the next call (E of released samples is fixed)
    _feed(js, dev, x, 150, 5)  # hi = 155, depth 0: [115, 150) is a released loss gap; now advance beyond hi in a silence
    js.silence([0], [160], [33])
    _go(js, dev, js._plan([0], mode="advance", upto=170))
    _go(js, dev, js._plan([0], mode="advance", upto=200))  # the silence in force continues over calls
    E = np.array(dev.out[0], dtype=np.float32)
    assert not E[135:150].any()  # (the loss gap [115, 150) outlasted the fade; the source [147, 155) of the next begins in it)
    assert np.array_equal(E[155:160], fade[:5] * np.concatenate([np.zeros(3, np.float32), x[150:152]])) and np.array_equal(_bits(E[160:200]), _bits(cn.samples(160, 40, 33)))
    assert js.export_slots([0]).tensors["jitter_cn_open"].tolist() == [33]


def test_silence_checks_everything_before_anything_changes():
    js = _host(S=2, seed=1)
    plan, pay = js._plan_feed([b""], [0], [1000])
    js._commit(plan.book)
    before = js.export_slots([0, 1])
    for args in (([0, 2], [0, 0], [1, 1]), ([0], [0, 1], [1]), ([0], [0], [1, 2]), ([0], [0], [128]), ([0], [0], [-1]), ([0], [0], [1.5]),
                 ([0], [0], [True]), ([0], [1 << 32], [5]), ([0], [0.5], [5]), ([True], [0], [5]), ([0, 0], [1000, 1001], [5, "5"])):
        with pytest.raises(ValueError):
            js.silence(*args)
        now = js.export_slots([0, 1])
        assert all(torch.equal(before.tensors[k], now.tensors[k]) for k in before.tensors)
    plain = _host(S=2, seed=None)
    with pytest.raises(ValueError, match="ComfortNoise"):
        plain.silence([0], [0], [5])
    from afx.jitter import JitterScorer, MixedJitterScorer
    for bad in (3, "cn", True):
        with pytest.raises(ValueError):
            JitterScorer(_inner(1), 8000, "mulaw", 160, comfort_noise=bad)
        with pytest.raises(ValueError):
            MixedJitterScorer(_inner(1), [(8000, "mulaw")], 20, comfort_noise=bad)
    js.silence(torch.tensor([0, 0]), np.array([1000, 1400]), np.array([5, 6]))
    assert js._b.marks == {0: [[0, 5], [400, 6]]} and js.stats()["marks"].tolist() == [2, 0]


# ---- no marks, no change ------------------------------------------------------------------------------------------------------------
def test_a_scorer_that_never_gets_a_mark_plans_what_a_scorer_without_comfort_noise_plans():
    rate, depth = 8000, 480
    a, b = _host(S=2, rate=rate, depth=depth, seed=5), _host(S=2, rate=rate, depth=depth, seed=None)
    ev = [[e for e in dtx_events(rate, 40 + s) if e[0] == "pkt"] for s in range(2)]
    rng = random.Random(3)
    n_ops = 0
    for i in range(max(len(e) for e in ev)):
        rows = [(s,) + ev[s][i][1:] for s in range(2) if i < len(ev[s])]
        rng.shuffle(rows)
        plans = [js._plan_feed([r[2].tobytes() for r in rows], [r[0] for r in rows], [r[1] for r in rows])[0] for js in (a, b)]
        if i % 9 == 4:
            plans += [js._plan([0, 1], mode="advance", upto=int(js.samples_in.max()) + 700) for js in (a, b)]
        for pa, pb in zip(plans[0::2], plans[1::2]):
            assert [op[0] for op in pa.ops] == [op[0] for op in pb.ops] and "noise" not in [op[0] for op in pa.ops]
            for oa, ob in zip(pa.ops, pb.ops):
                assert np.array_equal(oa[1], ob[1]) and oa[1].dtype == ob[1].dtype and oa[2] == ob[2]
            assert np.array_equal(pa.counts, pb.counts)
            n_ops += len(pa.ops)
            a._commit(pa.book)
            b._commit(pb.book)
    assert n_ops > 100 and a.stats()["concealed"].tolist() == b.stats()["concealed"].tolist() and a.stats()["concealed"].sum() > 0
    assert set(a.stats()) == set(b.stats()) | {"comfort", "marks", "marks_late"} and not a.stats()["comfort"].any()
    today = {"samples", "jitter_pending", "jitter_fill", "jitter_ring", "jitter_book", "jitter_stats", "jitter_intervals"}
    ex = b.export_slots([0, 1])
    assert set(ex.tensors) == today and "jitter_cn" not in ex.meta and "jitter_cn" not in b.state_meta()
    assert set(b.stats()) == {"received", "late", "duplicate", "concealed", "out_of_order"}
    exa = a.export_slots([0, 1])
    assert set(exa.tensors) == today | {"jitter_cn_marks", "jitter_cn_open", "jitter_cn_stats"} and exa.meta["jitter_cn"] == 5
    assert all(torch.equal(ex.tensors[k], exa.tensors[k]) for k in today) and a.state_meta() == exa.meta


# ---- RTP ------------------------------------------------------------------------------------------------------------------------------
def test_feed_rtp_takes_comfort_noise_and_ignored_types():
    from afx import rtp
    assert rtp.CN_PAYLOAD_TYPE == 13 and 13 not in rtp.STATIC_PAYLOAD_TYPES
    g = np.random.default_rng(0)
    pay = lambda: g.integers(0, 256, 160).astype(np.uint8).tobytes()
    plain = _host(S=2, encoding="mulaw", depth=160, seed=None)
    with pytest.raises(ValueError) as e13:
        plain.feed_rtp([_rtp(1, 0, pt=13, payload=b"\x28")], [0])
    with pytest.raises(ValueError) as e99:
        plain.feed_rtp([_rtp(1, 0, pt=99, payload=b"\x28")], [0])
    assert str(e13.value) == "slot 0: RTP payload type 13 is not this scorer's mulaw" == str(e99.value).replace("99", "13")
    with pytest.raises(ValueError, match="payload type 98 is not"):
        plain.feed_rtp([_rtp(1, 0, pt=98, payload=b"\x28")], [0], payload_types={98: "cn"})
    js = _host(S=2, encoding="mulaw", depth=160, seed=9)
    ref = _host(S=2, encoding="mulaw", depth=160, seed=9)
    dj, dr = NumpyDevice(js), NumpyDevice(ref)

    def snap(s):
        e = s.export_slots([0, 1])
        return [e.tensors[k] for k in sorted(e.tensors)] + list(s.stats().values())

    # refusals: nothing changes, wherever in the call the bad datagram stands
    a0 = pay()
    p, py, ssrc = js._plan_rtp([_rtp(1, 5000, payload=a0)], [0])
    _go(js, dj, p, py)
    js._b.ssrc[0] = ssrc[0]
    before = snap(js)
    cn1 = _rtp(2, 5160, pt=13, payload=b"\x32\x01\x02")  # level 50, then two reflection coefficients (read past)
    for dg, kw in (([cn1, _rtp(3, 5160, pt=13, payload=b"")], {}),  # an empty CN payload
                   ([cn1, _rtp(3, 5320, payload=pay(), ssrc=5)], {}),  # a foreign SSRC after a good mark
                   ([cn1, _rtp(3, 5320, pt=101, payload=b"\x01\x00\x00\xa0")], {}),  # telephone-event, not ignored
                   ([cn1, _rtp(3, 5320, pt=101, payload=b"\x01", ssrc=5)], dict(ignore_types=(101,))),  # ignored types are SSRC-checked
                   ([cn1, _rtp(3, 5320)[:9]], {}), ([cn1], dict(ignore_types=(300,))), ([cn1], dict(ignore_types=5)),
                   ([cn1, _rtp(3, 5320, pt=98, payload=b"\x10")], {})):
        with pytest.raises(ValueError):
            js.feed_rtp(dg, [0] * len(dg), **kw)
        assert all(torch.equal(x, y) for x, y in zip(before, snap(js))) and not js._b.marks and int(js._b.ssrc[0]) == 0x11223344
    assert int(js._b.ssrc[1]) == -1
    # marks alone plan no launch, so this runs on a host-only scorer; {98: "cn"} works; bit 7 of the level byte is masked
    res = js.feed_rtp([cn1, _rtp(3, 5200, pt=98, payload=b"\xff")], [0, 0], payload_types={98: "cn"})
    assert res.counts.tolist() == [0, 0] and js._b.marks == {0: [[160, 50], [200, 127]]}
    res = js.feed_rtp([_rtp(4, 5320, pt=101, payload=b"\x01\x00\x00\xa0")], [0], ignore_types=[101])
    assert res.counts.tolist() == [0] and _stats(js, 0)["received"] == 160
    # interleaved CN, telephone events and audio in one call == silence, then feed of the audio alone
    ref._commit(ref._plan_feed([a0], [0], [5000], seqs=[1])[0].book)
    dr.ring[:] = dj.ring
    dr.out, dr.N = [list(o) for o in dj.out], list(dj.N)
    ref.silence([0, 0], [5160, 5200], [50, 127])
    a1, a2, b1 = pay(), pay(), pay()
    dg = [_rtp(8, 6000, payload=a2), _rtp(6, 5520, pt=13, payload=b"\x46"), _rtp(1, 77, payload=b1, ssrc=3), _rtp(5, 5360, pt=101, payload=b"\x01"),
          _rtp(7, 5840, payload=a1), _rtp(2, 237, pt=13, payload=b"\x20", ssrc=3)]
    p, py, ssrc = js._plan_rtp(dg, [0, 0, 1, 0, 0, 1], ignore_types=(101,))
    assert ssrc == {0: 0x11223344, 1: 3} and p.counts.shape == (6,) and int(js._b.ssrc[1]) == -1
    _go(js, dj, p, py)
    ref.silence([0, 1], [5520, 237], [70, 32])  # (slot 1 has no session yet at that point: dropped in both)
    q, qy = ref._plan_feed([a2, b1, a1], [0, 1, 0], [6000, 77, 5840], seqs=[8, 1, 7])
    _go(ref, dr, q, qy)
    assert [op[0] for op in p.ops] == [op[0] for op in q.ops] and all(np.array_equal(x[1], y[1]) for x, y in zip(p.ops, q.ops))
    assert "noise" in [op[0] for op in p.ops] and p.counts.tolist() == [int(q.counts[0]), 0, int(q.counts[1]), 0, 0, 0]
    for s in (0, 1):
        assert np.array_equal(_bits(dj.out[s]), _bits(dr.out[s])) and _stats(js, s) == _stats(ref, s)
    assert _stats(js, 0)["comfort"] == 5840 - 5160 and _stats(js, 1)["marks_late"] == 1 and _stats(js, 0)["out_of_order"] == 1
    E = np.array(dj.out[0], dtype=np.float32)
    assert np.array_equal(_bits(E[160:200]), _bits(js.cn.samples(160, 40, 50))) and np.array_equal(_bits(E[520:840]), _bits(js.cn.samples(520, 320, 70)))


# ---- sessions ---------------------------------------------------------------------------------------------------------------------------
def test_a_session_exported_mid_silence_continues_in_another_scorer_and_the_refusals():
    from afx.streaming import StreamState
    P, F, depth = 8, 20, 30
    kw = dict(depth=depth, conceal="repeat", period=P, fade=F, ts_bits=None)
    A, B = _host(S=2, seed=11, **kw), _host(S=3, seed=11, max_pending=2, **kw)
    da, db = NumpyDevice(A), NumpyDevice(B)
    ref = RefSlot(depth, "repeat", P, F, noise=11)
    x = np.arange(1, 401, dtype=np.float32)

    def feed(js, dev, slot, t, n, marks=()):
        mk = ([slot] * len(marks), [m[0] for m in marks], [m[1] for m in marks]) if marks else None
        plan, pay = js._plan_feed([x[t:t + n].tobytes()], [slot], [t], marks=mk)
        _go(js, dev, plan, pay)
        for m in marks:
            ref.mark(*m)
        ref.packet(t, x[t:t + n])
        ref.after_feed()

    feed(A, da, 0, 0, 50)
    feed(A, da, 0, 115, 5, marks=[(56, 44), (100, 45), (130, 46)])  # hi = 120: [20, 90) released, noise from 56 on, at level 44
    assert int(A.samples_in[0]) == 90 == ref.next and ref.gap == 50 and ref.level == 44
    st = A.export_slots([0])
    assert st.tensors["jitter_book"][0].tolist()[:5] == [0, 1, 90, 120, 50] and st.meta["jitter_cn"] == 11
    assert st.tensors["jitter_cn_marks"].tolist() == [[[100, 45], [130, 46]]] and st.tensors["jitter_cn_open"].tolist() == [44]
    assert st.tensors["jitter_cn_stats"].tolist() == [[34, 3, 0]] and st.tensors["jitter_stats"][0, 3].item() == 6
    assert all(st.tensors[k].dtype == torch.int64 for k in ("jitter_cn_marks", "jitter_cn_open", "jitter_cn_stats"))
    B.import_slots([2], StreamState.from_state_dict(st.to("cpu").state_dict()))
    db.out[2], db.N[2] = list(da.out[0]), da.N[0]
    feed(B, db, 2, 160, 40)  # [90, 100) at 44, [100, 115) at 45, received, then [120, 130) loss and [130, 160) at 46
    feed(B, db, 2, 200, 60)
    assert np.array_equal(_bits(db.out[2]), _bits(ref.E)) and len(ref.E) == 230 and _stats(B, 2) == ref.stats
    E = np.array(ref.E, dtype=np.float32)
    assert np.array_equal(_bits(E[56:100]), _bits(A.cn.samples(56, 44, 44))) and np.array_equal(_bits(E[100:115]), _bits(A.cn.samples(100, 15, 45)))
    assert np.array_equal(_bits(E[130:160]), _bits(A.cn.samples(130, 30, 46))) and E[120:130].all() and ref.stats["comfort"] == 89
    assert int(A.samples_in[0]) == 90 and A._b.marks == {0: [[100, 45], [130, 46]]}  # the source went on untouched
    # a state with marks: refused by name without a ComfortNoise and with another seed; nothing changes
    plain, other = _host(S=2, seed=None, **kw), _host(S=2, seed=12, **kw)
    with pytest.raises(ValueError, match="jitter_cn.*no ComfortNoise"):
        plain.import_slots([1], st)
    with pytest.raises(ValueError, match="jitter_cn 11 is not this scorer's 12"):
        other.import_slots([1], st)
    assert not other._b.marks and other.samples_in.tolist() == [0, 0] and plain.samples_in.tolist() == [0, 0]
    # a plain state imports into a comfort-noise scorer with no marks, and goes on as a scorer that never saw one
    feedp = lambda t, n: plain._commit(plain._plan_feed([x[t:t + n].tobytes()], [0], [t])[0].book)
    feedp(0, 50)
    feedp(115, 5)
    other.silence([1], [0], [9])  # (dropped: no session; the counter is cleared by the import)
    other.import_slots([1], plain.export_slots([0]))
    assert other.samples_in.tolist() == [0, 90] and not other._b.marks and other._b.cn_open.tolist() == [-1, -1]
    assert _stats(other, 1) == dict(_stats(plain, 0), comfort=0, marks=0, marks_late=0)
    back = other.export_slots([1])
    assert back.tensors["jitter_cn_marks"].tolist() == [[[-1, -1]]] and back.tensors["jitter_cn_open"].tolist() == [-1]

    def edited(key, fn):
        t = {k: v.clone() for k, v in st.tensors.items()}
        fn(t[key])
        return StreamState(st.meta, st.seen, t)

    for bad in (edited("jitter_cn_open", lambda t: t.__setitem__(0, 128)), edited("jitter_cn_marks", lambda t: t[0, 0].__setitem__(0, 89)),
                edited("jitter_cn_marks", lambda t: t[0, 1].__setitem__(0, 100)), edited("jitter_cn_marks", lambda t: t[0, 0].__setitem__(1, 128)),
                edited("jitter_cn_stats", lambda t: t[0].__setitem__(0, 85)), edited("jitter_cn_stats", lambda t: t[0].__setitem__(1, 1)),
                StreamState(st.meta, st.seen, {k: v for k, v in st.tensors.items() if k != "jitter_cn_open"}),
                StreamState(st.meta, st.seen, dict(st.tensors, jitter_cn_open=st.tensors["jitter_cn_open"].int()))):
        with pytest.raises(ValueError):
            B.import_slots([0], bad)
    assert B.samples_in.tolist() == [0, 0, 230]


# ---- mixed rates ------------------------------------------------------------------------------------------------------------------------
def test_a_16_khz_slot_with_cn_on_a_dynamic_type_beside_8_khz_slots_equals_the_one_rate_scorer():
    from afx.jitter import ComfortNoise, JitterScorer, MixedJitterScorer
    cn = ComfortNoise(21)
    mx = MixedJitterScorer(_inner(3), [(8000, "mulaw"), (16000, "pcm_s16le")], 60, comfort_noise=cn)
    mx.reset([0, 1, 2], [8000, 16000, 8000])
    one = {s: JitterScorer(_inner(3), r, e, 60 * r // 1000, comfort_noise=cn) for s, (r, e) in
           enumerate([(8000, "mulaw"), (16000, "pcm_s16le"), (8000, "mulaw")])}
    dm, do = NumpyDevice(mx), {s: NumpyDevice(j) for s, j in one.items()}
    types = {97: (16000, "pcm_s16le"), 98: (16000, "cn")}
    own = {0: {}, 1: {97: "pcm_s16le", 98: "cn"}, 2: {}}
    g = np.random.default_rng(4)
    with pytest.raises(ValueError, match="8000 Hz, the slot is at 16000 Hz"):
        mx.feed_rtp([_rtp(1, 0, pt=13, payload=b"\x20")], [1], payload_types=types)  # 13 is CN at the 8 kHz clock
    with pytest.raises(ValueError):
        mx.feed_rtp([_rtp(1, 0, pt=98, payload=b"\x20")], [0], payload_types=types)
    with pytest.raises(ValueError):
        MixedJitterScorer(_inner(1), [(8000, "mulaw")], 60).feed_rtp([_rtp(1, 0, pt=13, payload=b"\x20")], [0])
    ev = {}
    for s, rate in ((0, 8000), (1, 16000), (2, 8000)):
        out = []
        for kind, t, v in dtx_events(rate, 300 + s, n_spurts=4):
            if kind == "cn":
                out.append((t, 98 if s == 1 else 13, bytes([v, 1, 2])))
            elif s == 1:
                out.append((t, 97, g.integers(-2000, 2000, len(v)).astype("<i2").tobytes()))
            else:
                out.append((t, 0, g.integers(0, 256, len(v)).astype(np.uint8).tobytes()))
        ev[s] = out
    at, seq = {s: 0 for s in ev}, {s: 0 for s in ev}
    rng = random.Random(8)
    step = 0
    while any(at[s] < len(ev[s]) for s in ev):
        step += 1
        rows = []
        for s in ev:
            if at[s] < len(ev[s]) and rng.random() < 0.8:
                m = rng.randint(1, 3)
                for t, pt, payload in ev[s][at[s]:at[s] + m]:
                    seq[s] += 1
                    rows.append((s, _rtp(seq[s] & 0xFFFF, (t + 1000 * s) % (1 << 32), pt=pt, payload=payload, ssrc=50 + s)))
                at[s] += m
        if step % 5 == 0:
            rows.append((0, _rtp(9, 0, pt=101, payload=b"\x05", ssrc=50)))
        if not rows:
            continue
        rng.shuffle(rows)
        pm, paym, ssrc = mx._plan_rtp([r[1] for r in rows], [r[0] for r in rows], payload_types=types, ignore_types=(101,))
        _go(mx, dm, pm, paym)
        for s, v in ssrc.items():
            mx._b.ssrc[s] = v
        for s in sorted({r[0] for r in rows}):
            mine = [i for i, r in enumerate(rows) if r[0] == s]
            p1, pay1, ss = one[s]._plan_rtp([rows[i][1] for i in mine], [s] * len(mine), payload_types=own[s], ignore_types=(101,))
            _go(one[s], do[s], p1, pay1)
            one[s]._b.ssrc[s] = ss[s]
            assert pm.counts[mine].tolist() == p1.counts.tolist()  # call for call
            assert np.array_equal(_bits(dm.out[s]), _bits(do[s].out[s])) and _stats(mx, s) == _stats(one[s], s), (step, s)
            assert int(mx.samples_in[s]) == int(one[s].samples_in[s]) and int(mx.pending[s]) == int(one[s].pending[s])
    for s in ev:
        assert _stats(mx, s)["comfort"] > 0 and _stats(mx, s)["marks"] > 0 and _stats(mx, s)["received"] > 0
    assert dm.noise_rows > 10
    # a session of the one-rate scorer at a listed rate moves in mid-stream, marks and all; and between mixed scorers
    st = one[1].export_slots([1])
    mx2 = MixedJitterScorer(_inner(2), [(16000, "pcm_s16le"), (8000, "mulaw")], 60, comfort_noise=cn)
    mx2.import_slots([0], st)
    mx2.import_slots([1], mx.export_slots([2]))
    assert mx2.rates.tolist() == [16000, 8000] and _stats(mx2, 0) == _stats(one[1], 1) and _stats(mx2, 1) == _stats(mx, 2)
    assert mx2._b.marks.get(0) == one[1]._b.marks.get(1) and mx2._b.cn_open.tolist() == [int(one[1]._b.cn_open[1]), int(mx._b.cn_open[2])]
    with pytest.raises(ValueError, match="no ComfortNoise"):
        MixedJitterScorer(_inner(2), [(16000, "pcm_s16le"), (8000, "mulaw")], 60).import_slots([0], st)
    with pytest.raises(ValueError, match="jitter_cn"):
        MixedJitterScorer(_inner(2), [(16000, "pcm_s16le")], 60, comfort_noise=ComfortNoise(22)).import_slots([0], mx.export_slots([1]))


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------------
def test_noise_entry_points_are_in_header_library_and_ctypes_table_and_refuse_on_the_host(built):
    _lib = built
    src = open(os.path.join(ROOT, "include", "afx.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("afx_k_jitter_noise", "afx_k_jitter_noise_rates"):
        assert re.search(r"\b%s\s*\(" % name, src) and hasattr(lib, name) and name in _lib.SIGNATURES
    l = _lib.lib()
    buf = (ctypes.c_float * 128)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    table = (_lib.JitterRate * 2)()
    for t, J in zip(table, (16, 24)):
        t.taps, t.fade, t.L, t.M, t.T, t.J, t.P, t.F = None, None, 1, 1, 1, J, 0, 0
    tp = ctypes.cast(table, ctypes.c_void_p)
    # refused on the host: nothing is launched (there is no GPU here to launch on); each refusal names its entry point
    for args, word in (((None, 1, 16, p, 1, 1, 0, p, None), b"null"), ((p, 1, 16, None, 1, 1, 0, p, None), b"null"),
                       ((p, 1, 16, p, 1, 1, 0, None, None), b"amplitude"), ((p, 1, 16, p, 0, 1, 0, p, None), b"rows"),
                       ((p, 1, 16, p, 65536, 1, 0, p, None), b"rows"), ((p, 1, 16, p, 1, 17, 0, p, None), b"fit"),
                       ((p, 1, 16, p, 1, -1, 0, p, None), b"fit"), ((p, 0, 16, p, 1, 1, 0, p, None), b"fit")):
        assert l.afx_k_jitter_noise(*args) != 0 and b"jitter_noise:" in l.afx_last_error() and word in l.afx_last_error(), args
    for args, word in (((None, 1, 24, p, 1, 1, tp, 2, 0, p, None), b"null"), ((p, 1, 24, p, 1, 1, tp, 2, 0, None, None), b"amplitude"),
                       ((p, 1, 24, p, 1, 25, tp, 2, 0, p, None), b"fit"), ((p, 1, 24, p, 1, 1, None, 2, 0, p, None), b"null rate table"),
                       ((p, 1, 24, p, 1, 1, tp, 17, 0, p, None), b"1 to 16 rates"), ((p, 1, 20, p, 1, 1, tp, 2, 0, p, None), b"J <= Js"),
                       ((p, 1, 24, p, 0, 1, tp, 2, 0, p, None), b"rows")):
        assert l.afx_k_jitter_noise_rates(*args) != 0 and b"jitter_noise_rates:" in l.afx_last_error() and word in l.afx_last_error(), args
