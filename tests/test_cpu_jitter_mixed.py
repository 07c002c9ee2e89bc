"""Every slot its own clock rate in one jitter buffer (afx/jitter.py MixedJitterScorer), without a GPU.  The three new entry
points (afx_k_jitter_place_rates / _conceal_rates / _release_rates) are restated in numpy exactly as include/afx.h states
them (oracle/jitter.py's ``NumpyDevice``), on the host-only scorer's own ring, from the host table the launches would take; what
a slot releases must equal the per-sample simulation of its played-out stream E (its ``RefSlot``) bit for bit, with its counters, whatever the other slots' rates.  Also: a
slot wraps its ring at its own J and leaves the columns beyond it alone, the plan for a pool all at one rate is the one-rate
``JitterScorer``'s plan with a rate column, the checks and refusals (each leaving the scorer unchanged), the state an export
adds with the cross-refusals, and the new entry points in the header, the library and the ctypes table."""
import ctypes
import os
import random
import re

import numpy as np
import pytest
import torch

import packet_helpers
from oracle.jitter import NumpyDevice, RefSlot, Schedule as _Schedule, packet, per_packet, rtp as _rtp, sizing as _sizing
from packet_helpers import bits as _bits, go as _go, inner as _inner, same as _same, snap as _snap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 4000
FORMATS = [(8000, "mulaw"), (8000, "alaw"), (11025, "pcm_s16le"), (16000, "pcm_f32le"), (48000, "pcm_s16le")]
ENC_AT = {8000: ("mulaw", "alaw"), 11025: ("pcm_s16le",), 16000: ("pcm_f32le",), 48000: ("pcm_s16le",)}
SLOT_RATES = [8000, 11025, 16000, 48000, 8000, 48000]
DEPTH_MS = 60


def _packet(encoding, n, g):
    return packet(encoding, n, g, amp=1.0, div=1)  # full-scale noise


def Schedule(rate, encodings, seed, jump=0, P=0, **kw):
    return _Schedule(rate, encodings, seed, jump=jump, short=max(1, P // 2), payload=per_packet(amp=1.0, div=1), **kw)


@pytest.fixture(scope="module", autouse=True)
def built():
    return packet_helpers.built()


def _mixed(S=6, formats=FORMATS, depth_ms=DEPTH_MS, rates=None, **kw):
    from afx.jitter import MixedJitterScorer
    ms = MixedJitterScorer(_inner(S), formats, depth_ms, **kw)
    if rates is not None:
        ms.reset(list(range(S)), rates)
    return ms


def _plain(S, rate, mode="repeat", depth_ms=DEPTH_MS, **kw):
    """The one-rate scorer of the contract for ``rate``."""
    from afx.jitter import JitterScorer
    depth, P, F, _, _, _ = _sizing(rate, mode, depth_ms)
    return JitterScorer(_inner(S), rate, ENC_AT[rate], depth, conceal=mode, period=P or None, fade=F if mode == "repeat" else None, **kw)


SENTINEL = np.float32(-7.25)


@pytest.mark.parametrize("mode", ["repeat", "zero"])
def test_placement_playout_and_concealment_of_every_rate_equal_a_per_sample_simulation(mode):
    S = 6
    ms = _mixed(S, rates=SLOT_RATES, conceal=mode, ts_bits=32)
    geo = [_sizing(r, mode) for r in SLOT_RATES]
    depth, P, F, lookback, W, J = ([g[i] for g in geo] for i in range(6))
    # the sizing: per rate exactly the one-rate scorer's values, one ring as wide as the widest
    for s, r in enumerate(SLOT_RATES):
        one = _plain(1, r, mode)
        assert (one.depth, one.period, one.fade_len, one.lookback, one.W, one.J) == geo[s]
    assert (ms.rates.tolist(), ms.depths.tolist(), ms.periods.tolist(), ms.fades.tolist()) == (SLOT_RATES, depth, P, F)
    assert ms.Js == max(J) and tuple(ms.jring.shape) == (S, max(J)) and len(set(J)) == 4 and ms.delays.tolist()[2] == 0.0
    dev = NumpyDevice(ms)
    assert [r["J"] for r in dev.rate] == [J[0], J[1], J[2], J[3]]
    for s in range(S):  # the columns at and beyond a slot's own J keep what stands there
        dev.ring[s, J[s]:] = SENTINEL
    rng = random.Random(5 + len(mode))
    Pn = [r // 100 for r in SLOT_RATES]  # the traffic is made for the 10-ms period and its 30-ms fade in either mode
    Fn = [3 * p for p in Pn]
    sch = [Schedule(r, ENC_AT[r], 31 * s + len(mode), jump=J[s] + 123 + s, P=Pn[s], origin=(1 << 32) - 3000 if s in (1, 3) else None)
           for s, r in enumerate(SLOT_RATES)]
    assert set(sch[0].enc) == {"mulaw", "alaw"}
    refs = [RefSlot(depth[s], mode, P[s], F[s]) for s in range(S)]
    while not all(sc.done() for sc in sch):
        ticks = {s: sch[s].tick() for s in range(S) if not sch[s].done() and rng.random() < 0.8}
        if not ticks:
            continue
        order = [s for s, r in ticks.items() for _ in r]
        rng.shuffle(order)
        its = {s: iter(r) for s, r in ticks.items()}
        rows = [(s,) + next(its[s]) for s in order]
        before = _snap(ms)
        plan, pay = ms._plan_feed([r[3] for r in rows], [r[0] for r in rows], [r[1] for r in rows], encodings=[r[5] for r in rows])
        assert _same(before, _snap(ms))  # planning changes nothing
        _go(ms, dev, plan, pay)
        for s, ts, t, raw, x, e in rows:
            refs[s].packet(t, x)
        for s in ticks:
            refs[s].after_feed()
    plan = ms._plan(list(range(S)), mode="flush")
    _go(ms, dev, plan)
    st = ms.stats()
    for s in range(S):
        r = refs[s]
        r.release(r.hi)
        assert np.array_equal(_bits(dev.out[s]), _bits(r.E)), s
        assert int(ms.samples_in[s]) == r.next == dev.N[s] and int(ms.buffered[s]) == 0
        got = {k: int(v[s]) for k, v in st.items()}
        assert got == r.stats, (s, r.stats)
        # the traffic: two gaps closer than P in one release, a gap longer than F + P, a jump beyond the slot's own J, duplicates
        assert any(len(g) >= 2 and any(b[0] - a[1] < Pn[s] for a, b in zip(g, g[1:])) for g in r.releases)
        lens = [e - a for a, e in r.spans]
        assert max(lens) > J[s] and sum(1 for n in lens if Fn[s] + Pn[s] < n < J[s]) >= 1 and r.stats["duplicate"] > 0
        assert len(sch[s].lost) >= 6 and got["out_of_order"] > 0
        if mode == "repeat":  # concealed samples are there, and they are not zeros
            a, e = next((a, e) for a, e in r.spans if a >= 10 * (SLOT_RATES[s] // 50))
            assert np.count_nonzero(r.E[a:min(e, a + F[s])]) > 0.8 * min(e - a, F[s]) - 1
        # the slot wrapped its ring at its own J (several times) and never touched a column at or beyond it
        assert r.next > 2 * J[s] and (dev.ring[s, J[s]:] == SENTINEL).all()
    assert "conceal" in dev.launches and dev.launches.count("place") > 50


@pytest.mark.parametrize("rate", [8000, 11025, 16000, 48000])
def test_a_pool_all_at_one_rate_plans_the_one_rate_scorers_rows(rate):
    S = 3
    ms = _mixed(S, rates=rate)
    js = _plain(S, rate)
    ri = [8000, 11025, 16000, 48000].index(rate)
    P, J = _sizing(rate)[1], _sizing(rate)[5]
    sch = [Schedule(rate, ENC_AT[rate], 900 + s, jump=J + 50 if s == 1 else 0, P=P) for s in range(S)]
    rng = random.Random(rate)
    kinds = set()
    while not all(sc.done() for sc in sch):
        rows = [(s,) + r for s in range(S) if not sch[s].done() and rng.random() < 0.8 for r in sch[s].tick()]
        if not rows:
            continue
        rng.shuffle(rows)
        args = ([r[3] for r in rows], [r[0] for r in rows], [r[1] for r in rows])
        a, pa = ms._plan_feed(*args, encodings=[r[5] for r in rows])
        b, pb = js._plan_feed(*args, encodings=[r[5] for r in rows])
        assert [op[0] for op in a.ops] == [op[0] for op in b.ops] and a.counts.tolist() == b.counts.tolist() and a.slots == b.slots
        for x, y in zip(a.ops, b.ops):
            kinds.add(x[0])
            if x[0] == "pop":
                assert np.array_equal(x[1], y[1]) and x[2] == y[2]
                continue
            w = {"place": 5, "conceal": 4, "release": 7}[x[0]]
            assert np.array_equal(x[1][:, :w], y[1][:, :w]) and (x[1][:, -1] == ri).all() and x[2] == y[2] and x[1].dtype == np.int32
            assert x[1].shape[1] == w + 1 and (x[0] != "release" or not y[1][:, 7].any())
        ms._commit(a.book)
        js._commit(b.book)
    a, b = ms._plan(list(range(S)), mode="flush"), js._plan(list(range(S)), mode="flush")
    assert all(np.array_equal(x[1][:, :7], y[1][:, :7]) for x, y in zip(a.ops, b.ops) if x[0] == "release") and len(a.ops) == len(b.ops)
    assert kinds == {"place", "conceal", "release", "pop"}


def test_a_feed_naming_every_rate_is_one_place_one_release_and_one_pop_per_round():
    S = 6
    ms = _mixed(S, rates=SLOT_RATES)
    dev = NumpyDevice(ms)
    g = np.random.default_rng(0)
    encs = [ENC_AT[r][0] for r in SLOT_RATES]
    order = [3, 0, 5, 2, 4, 1]
    popped = 0
    for k in range(4):  # 250 ms per slot and feed: a hop of output each
        n = [r // 4 for r in SLOT_RATES]
        plan, pay = ms._plan_feed([_packet(encs[s], n[s], g)[0] for s in order], order, [k * n[s] for s in order])
        kinds = [op[0] for op in plan.ops]
        assert kinds in (["place", "release"], ["place", "release", "pop"]), kinds
        assert all(len(op[1]) == S for op in plan.ops) and sorted(set(plan.ops[1][1][:, 7].tolist())) == [0, 1, 2, 3]
        assert plan.ops[0][1][:, 5].tolist() == [ms._rate_of[s] for s in order]
        popped += kinds.count("pop")
        _go(ms, dev, plan, pay)
    assert popped == 3 and ms.samples_in.tolist() == [4 * (r // 4) - DEPTH_MS * r // 1000 for r in SLOT_RATES]


def test_timestamps_unwrap_across_two_to_the_32_in_a_48_khz_slot():
    ms = _mixed(2, formats=[(8000, "mulaw"), (48000, "pcm_s16le")], rates=[48000, 8000])
    dev = NumpyDevice(ms)
    g = np.random.default_rng(5)
    n_pk, size = 40, 960
    x = g.integers(-3000, 3000, n_pk * size).astype("<i2")
    start = (1 << 32) - 11 * size - 3  # the stream crosses 2**32 in its twelfth packet
    order = list(range(n_pk))
    rng = random.Random(5)
    for i in range(0, n_pk, 3):  # reordering within the depth
        blk = order[i:i + 3]
        rng.shuffle(blk)
        order[i:i + 3] = blk
    for k in order:
        t = (start + k * size) % (1 << 32)
        plan, pay = ms._plan_feed([x[k * size:(k + 1) * size].tobytes()], [0], [t])
        _go(ms, dev, plan, pay)
    _go(ms, dev, ms._plan([0], mode="flush"))
    assert np.array_equal(_bits(dev.out[0]), _bits(x.astype(np.float32) / np.float32(32768)))
    st = ms.stats()
    assert int(st["late"][0]) == 0 and int(st["concealed"][0]) == 0 and int(st["out_of_order"][0]) > 5
    assert ms.export_slots([0]).tensors["jitter_book"][0, 0].item() == start


# ---- checks and refusals -------------------------------------------------------------------------------------------------
def test_constructor_refusals_and_per_slot_properties():
    from afx.jitter import MixedJitterScorer
    sc = _inner(2)
    good = dict(formats=FORMATS, depth_ms=60)
    for kw in (dict(formats=[]), dict(formats=[(8000 + i, "mulaw") for i in range(17)]), dict(formats=[(8000, "mulaw"), (8000, "mulaw")]),
               dict(formats=[(7999, "mulaw")]), dict(formats=[(8000, "g722")]), dict(formats="mulaw"), dict(formats=[8000]),
               dict(depth_ms=-1), dict(depth_ms=1.5), dict(depth_ms=True), dict(period_ms=-1), dict(period_ms=2.5), dict(fade_ms=-1),
               dict(fade_ms=True), dict(conceal="pitch"), dict(max_pending=0), dict(ts_bits=3),
               dict(depth_ms=(1 << 30) * 1000 // 48000 + 1)):  # Js >= 2**30
        with pytest.raises(ValueError):
            MixedJitterScorer(sc, **dict(good, **kw))
    ms = MixedJitterScorer(sc, FORMATS, 60, period_ms=5, fade_ms=20)
    assert ms.rates.tolist() == [8000, 8000] and ms.periods.tolist() == [40, 40] and ms.fades.tolist() == [160, 160]  # the first format's rate
    ms.reset([1], 11025)
    assert (ms.depths.tolist(), ms.periods.tolist(), ms.fades.tolist()) == ([480, 661], [40, 55], [160, 220]) and ms.delays.tolist()[0] == 20.0
    z = MixedJitterScorer(sc, FORMATS, 60, conceal="zero", period_ms=5)
    assert z.periods.tolist() == [0, 0] and z.fades.tolist() == [0, 0]
    tiny = MixedJitterScorer(sc, [(8000, "mulaw")], 0, period_ms=0, fade_ms=0)
    assert tiny.periods.tolist() == [1, 1] and tiny.fades.tolist() == [0, 0]  # P_r = max(1, ...)
    for name, plural in (("delay", "delays"), ("depth", "depths"), ("period", "periods"), ("input_rate", "rates")):
        with pytest.raises(AttributeError, match=plural):
            getattr(ms, name)


def test_refusals_leave_a_host_scorer_unchanged():
    from afx._lib import AfxError
    ms = _mixed(4, formats=[(8000, "mulaw"), (8000, "alaw"), (16000, "pcm_s16le"), (48000, "pcm_s16le")], rates=[8000, 16000, 48000, 8000])
    pk8, pk16 = bytes(160), np.zeros(320, dtype=np.int16)
    plan, pay = ms._plan_feed([pk16.tobytes()], [1], [77])  # give slot 1 a session without a GPU: a packet inside the depth
    assert [op[0] for op in plan.ops] == ["place"]
    ms._commit(plan.book)
    before = _snap(ms)
    calls = [
        lambda: ms.reset([0], 22050), lambda: ms.reset([0, 1], [8000, 44100]), lambda: ms.reset([0, 1], [8000]), lambda: ms.reset([0], "8000"),
        lambda: ms.reset([0], 8000.0), lambda: ms.reset([0], True), lambda: ms.reset([0, 0], 8000), lambda: ms.reset([4], 8000),
        lambda: ms.feed([pk8], [0], [0], encodings=["pcm_s16le"]),  # listed, but at another rate than the slot's
        lambda: ms.feed([pk16], [1], [0], encodings=["mulaw"]), lambda: ms.feed([pk8], [0], [0], encodings=["g722"]),
        lambda: ms.feed([pk8], [0], [0], encodings="mulaw"), lambda: ms.feed([pk8], [0], [0], encodings=["mulaw", "alaw"]),
        lambda: ms.feed([pk8, pk8], [0], [0]), lambda: ms.feed([pk8], [0, 3], [0, 0]), lambda: ms.feed([pk8], [4], [0]),
        lambda: ms.feed([bytes(3)], [1], [0]),  # splits a 16-bit sample: slot 1's default is pcm_s16le
        lambda: ms.feed([pk8], [0], [0.5]), lambda: ms.feed([pk8], [0], [1 << 32]), lambda: ms.feed(pk8, [0], [0]),
        lambda: ms.feed([np.zeros(4 * H + 2000, dtype=np.int16)], [1], [0], score=False),
        lambda: ms.feed_rtp([_rtp(1, 0, pt=0, payload=pk8)], [1]),  # PT 0 is (8000, mulaw); slot 1 is at 16 kHz
        lambda: ms.feed_rtp([_rtp(1, 0, pt=96, payload=pk8)], [0]),  # an unknown type
        lambda: ms.feed_rtp([_rtp(1, 0, pt=96, payload=pk8)], [0], payload_types={96: (8000, "pcm_s16le")}),  # not listed
        lambda: ms.feed_rtp([_rtp(1, 0, pt=96, payload=pk8)], [0], payload_types={96: (16000, "pcm_s16le")}),  # another rate than the slot's
        lambda: ms.feed_rtp([_rtp(1, 0, pt=96, payload=pk8)], [0], payload_types={96: "mulaw"}),  # a pair is asked for
        lambda: ms.feed_rtp([_rtp(1, 0, payload=pk8), _rtp(2, 160, payload=pk8, ssrc=5)], [0, 0]),
        lambda: ms.feed_rtp([_rtp(1, 0, payload=pk8)[:8]], [0]),
        lambda: ms.drain([4]), lambda: ms.flush([0, 0]), lambda: ms.advance([0], 5), lambda: ms.advance([1], -1), lambda: ms.advance([1], [1, 2]),
    ]
    for i, call in enumerate(calls):
        with pytest.raises(ValueError):
            call()
        assert _same(before, _snap(ms)), i
    for call in (lambda: ms.feed([pk8, pk16], [0, 1], [0, 157]), lambda: ms.flush([1]), lambda: ms.advance([1], 10)):
        with pytest.raises(AfxError):  # valid, but there is no GPU behind this scorer: nothing changes either
            call()
        assert _same(before, _snap(ms))
    # empty payloads plan no launch, so these run on a host-only scorer: PT 8 into an 8 kHz slot, a dynamic type at 16 kHz
    ms.feed_rtp([_rtp(65535, 0, pt=8), _rtp(1, 320, pt=0), _rtp(0, 160, pt=8)], [0, 0, 0])
    ms.feed_rtp([_rtp(9, 500, pt=97, ssrc=7)], [1], payload_types={97: (16000, "pcm_s16le")})
    assert int(ms.stats()["out_of_order"][0]) == 1 and ms.export_slots([0]).tensors["jitter_book"][0].tolist()[6:] == [1, 0x11223344]
    with pytest.raises(ValueError):
        ms.feed_rtp([_rtp(2, 480, pt=0, ssrc=7)], [0])  # not the session's SSRC
    res = ms.feed([b"", bytearray()], [2, 0], [500, 0])
    assert res.counts.tolist() == [0, 0] and ms.feed([], [], []).counts.tolist() == [] and ms.drain().counts.tolist() == [0] * 4
    ms.reset([1, 0], [48000, 16000])  # a reset with rates: per slot, in the order named
    assert ms.rates.tolist() == [16000, 48000, 48000, 8000] and ms.buffered.tolist() == [0] * 4 and not ms.stats()["out_of_order"].any()
    ms.reset([2])  # None keeps the slot's rate
    assert ms.rates.tolist() == [16000, 48000, 48000, 8000]


# ---- state -----------------------------------------------------------------------------------------------------------------
def test_state_keys_meta_params_and_cross_refusals():
    from afx.jitter import JITTER_FORMAT
    from afx.streaming import StreamState
    fm = [(8000, "mulaw"), (48000, "pcm_s16le"), (16000, "pcm_s16le")]
    ms = _mixed(3, formats=fm, rates=[48000, 8000, 16000], max_pending=3)
    g = np.random.default_rng(1)
    for s, t, n, e in ((0, 100, 960, "pcm_s16le"), (0, 100 + 1920, 960, "pcm_s16le"), (1, 7, 80, "mulaw")):  # slot 0 holds a hole
        plan, pay = ms._plan_feed([_packet(e, n, g)[0]], [s], [t])
        assert all(op[0] == "place" for op in plan.ops)
        NumpyDevice(ms).run(plan, pay)
        ms._commit(plan.book)
    st = ms.export_slots([1, 0])
    assert set(st.tensors) == {"samples", "jitter_pending", "jitter_fill", "jitter_ring", "jitter_book", "jitter_stats",
                               "jitter_intervals", "jitter_rate", "jitter_params"}
    assert st.tensors["jitter_rate"].tolist() == [8000, 48000] and st.tensors["jitter_params"].tolist() == [[480, 80, 240], [2880, 480, 1440]]
    assert st.tensors["jitter_rate"].dtype == torch.int64 and st.tensors["jitter_params"].dtype == torch.int64
    lb8, lb48 = _sizing(8000)[3], _sizing(48000)[3]
    assert tuple(st.tensors["jitter_ring"].shape) == (2, lb48 + 2880) and lb48 + 2880 > lb8 + 480  # the widest of the scorer's rates
    ring = st.tensors["jitter_ring"]
    assert ring[0, lb8:lb8 + 80].any() and not ring[0, lb8 + 80:].any() and not ring[0, :lb8].any()  # zero beyond the session's own
    assert ring[1, lb48:lb48 + 960].any() and not ring[1, lb48 + 960:lb48 + 1920].any() and ring[1, lb48 + 1920:].any()
    assert st.tensors["jitter_intervals"].tolist() == [[[0, 80], [-1, -1]], [[0, 960], [1920, 2880]]]
    want = dict(resampler="kaiser5-hl10", jitter=JITTER_FORMAT, jitter_conceal="repeat", jitter_mixed=1)
    assert {k: st.meta[k] for k in want} == want and ms.state_meta() == st.meta
    assert not {"input_rate", "jitter_depth", "jitter_period", "jitter_fade", "encoding"} & set(st.meta)
    # into another mixed scorer: other formats order, other encodings, another S and max_pending
    other = _mixed(4, formats=[(16000, "pcm_f32le"), (48000, "pcm_f32le"), (8000, "alaw")], max_pending=1)
    other.import_slots([3, 1], StreamState.from_state_dict(st.to("cpu").state_dict()))
    back = other.export_slots([3, 1])
    assert all(torch.equal(back.tensors[k], st.tensors[k]) for k in st.tensors if k != "jitter_pending")
    assert other.rates.tolist() == [16000, 48000, 16000, 8000] and other.buffered.tolist() == [0, 2880, 0, 80]
    assert not other.jring[3, _sizing(8000)[5]:].any()
    # a plain JitterScorer's state is accepted where its rate is listed and its parameters are that rate's here
    plain = _plain(2, 48000)
    p2, pay = plain._plan_feed([_packet("pcm_s16le", 960, g)[0]], [1], [5], encodings=["pcm_s16le"])
    NumpyDevice(plain).run(p2, pay)
    plain._commit(p2.book)
    pst = plain.export_slots([1])
    other.import_slots([0], pst)
    assert other.rates.tolist()[0] == 48000 and int(other.buffered[0]) == 960
    e0 = other.export_slots([0])
    assert torch.equal(e0.tensors["jitter_ring"][:, :pst.tensors["jitter_ring"].shape[1]], pst.tensors["jitter_ring"])
    assert torch.equal(e0.tensors["jitter_book"], pst.tensors["jitter_book"])
    # the cross-refusals, each before anything changes
    keep = _snap(ms)
    keep_plain = _snap(plain)
    with pytest.raises(ValueError):
        plain.import_slots([0, 1], st)  # a mixed state into a plain JitterScorer
    with pytest.raises(ValueError):
        _plain(2, 8000).import_slots([0], ms.export_slots([1]))
    assert _same(keep_plain, _snap(plain))

    def edited(key, fn, base=st):
        t = {k: v.clone() for k, v in base.tensors.items()}
        fn(t[key])
        return StreamState(base.meta, base.seen, t)

    def set_(r, c, v):
        return lambda t: t[r].__setitem__(c, v)

    foreign = [
        _mixed(2, formats=[(8000, "mulaw"), (22050, "pcm_s16le")], rates=[8000, 22050]).export_slots([0, 1]),  # an unlisted rate
        _mixed(2, formats=fm, depth_ms=61, rates=[8000, 48000]).export_slots([0, 1]),  # parameters that differ: depth
        _mixed(2, formats=fm, period_ms=5, rates=[8000, 48000]).export_slots([0, 1]),  # period (and fade)
        _mixed(2, formats=fm, fade_ms=31, rates=[8000, 48000]).export_slots([0, 1]),
        _mixed(2, formats=fm, conceal="zero", rates=[8000, 48000]).export_slots([0, 1]),
        _plain(2, 11025).export_slots([0, 1]),  # a plain state at an unlisted rate
        _plain(2, 48000, depth_ms=61).export_slots([0, 1]), _plain(2, 48000, mode="zero").export_slots([0, 1]),
        _inner(2).export_slots([0, 1]), st.tensors, None,
        edited("jitter_ring", set_(0, lb8 + 480, 1.0)),  # non-zero beyond the 8 kHz session's own columns
        edited("jitter_ring", lambda t: None, base=StreamState(st.meta, st.seen, dict(st.tensors, jitter_ring=st.tensors["jitter_ring"][:, :lb48]))),
        edited("jitter_rate", lambda t: t.__setitem__(0, 48000)),  # the 8 kHz session's parameters are not 48 kHz's
        edited("jitter_params", set_(0, 0, 481)),
        StreamState(st.meta, st.seen, dict(st.tensors, jitter_rate=st.tensors["jitter_rate"].to(torch.int32))),
        edited("jitter_book", set_(0, 2, 5)), edited("jitter_book", set_(1, 3, 2881)), edited("jitter_book", set_(0, 4, 3)),
        edited("jitter_stats", set_(1, 1, -1)), edited("jitter_fill", lambda t: t.__setitem__(0, 1)),
        edited("jitter_intervals", lambda t: t[1, 1].__setitem__(0, 900)),
        StreamState(dict(st.meta, resampler="other"), st.seen, st.tensors), StreamState(dict(st.meta, jitter=JITTER_FORMAT + 1), st.seen, st.tensors),
    ]
    for i, f in enumerate(foreign):
        with pytest.raises(ValueError):
            ms.import_slots([0, 1], f)
        assert _same(keep, _snap(ms)), i
    with pytest.raises(ValueError):
        ms.import_slots([0], st)  # two sessions for one slot
    assert _same(keep, _snap(ms))


def test_a_session_exported_mid_gap_continues_in_another_mixed_scorer_at_its_own_rate():
    from afx.streaming import StreamState
    fm = [(8000, "mulaw"), (11025, "pcm_s16le")]
    A, B = _mixed(2, formats=fm, rates=[11025, 8000]), _mixed(3, formats=fm[::-1], max_pending=2)
    da, db = NumpyDevice(A), NumpyDevice(B)
    depth, P, F, lb, W, J = _sizing(11025)
    ref = RefSlot(depth, "repeat", P, F)
    g = np.random.default_rng(2)
    n = 11025 // 50
    raw, x = _packet("pcm_s16le", 40 * n, g)

    def feed(js, dev, slot, k):
        plan, pay = js._plan_feed([raw[2 * k * n:2 * (k + 1) * n]], [slot], [k * n])
        _go(js, dev, plan, pay)
        ref.packet(k * n, x[k * n:(k + 1) * n])
        ref.after_feed()

    for k in list(range(10)) + [12, 13]:  # hi = 14 packets, the playout point 11 packets: inside the gap that began at 10
        feed(A, da, 0, k)
    assert int(A.samples_in[0]) == ref.next == 14 * n - depth and ref.gap == 10 * n
    st = A.export_slots([0])
    assert st.tensors["jitter_book"][0].tolist()[2:5] == [ref.next, 14 * n, 10 * n] and st.tensors["jitter_rate"].tolist() == [11025]
    assert np.array_equal(st.tensors["jitter_ring"][0, :lb].numpy(), np.array(ref.E[ref.next - lb:], dtype=np.float32))
    B.import_slots([2], StreamState.from_state_dict(st.to("cpu").state_dict()))
    assert B.rates.tolist() == [11025, 11025, 11025] and int(B.samples_in[2]) == ref.next
    db.out[2], db.N[2] = list(da.out[0]), da.N[0]
    feed(B, db, 2, 11)  # inside the open gap, ahead of the playout point: placed, not late
    for k in range(14, 40):
        if k not in (20, 21, 22, 23, 30):
            feed(B, db, 2, k)
    _go(B, db, B._plan([2], mode="flush"))
    ref.release(ref.hi)
    assert np.array_equal(_bits(db.out[2]), _bits(ref.E)) and len(ref.E) == 40 * n and ref.next > 2 * J
    assert {k: int(v[2]) for k, v in B.stats().items()} == ref.stats and ref.stats["late"] == 0 and ref.stats["concealed"] == 6 * n
    assert int(A.samples_in[0]) == 14 * n - depth  # the source went on untouched


# ---- the entry points ------------------------------------------------------------------------------------------------------
def test_rate_entry_points_are_in_header_library_and_ctypes_table_and_refuse_on_the_host(built):
    _lib = built
    src = open(os.path.join(ROOT, "include", "afx.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    names = ("afx_k_jitter_place_rates", "afx_k_jitter_conceal_rates", "afx_k_jitter_release_rates")
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, src) and hasattr(cdll, name) and name in _lib.SIGNATURES
    assert "afx_jitter_rate" in src and ctypes.sizeof(_lib.JitterRate) == 40
    l = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    most = (ctypes.c_int * 16)(*([1] * 16))

    def table(n=1, **kw):
        t = (_lib.JitterRate * max(n, 1))()
        for e in t:
            e.taps, e.fade, e.L, e.M, e.T, e.J, e.P, e.F = p.value, p.value, 1, 2, 8, 64, 8, 16
            for k, v in kw.items():
                setattr(e, k, v)
        return ctypes.cast(t, ctypes.c_void_p), t

    def place(t, n=1, stage=p, hdr=p, rows=1, max_n=1, jring=p, Js=64):
        return l.afx_k_jitter_place_rates(stage, 64, hdr, rows, max_n, t, n, jring, 1, Js, None)

    def conceal(t, n=1, jring=p, hdr=p, rows=1, max_n=1, mode=1, Js=64):
        return l.afx_k_jitter_conceal_rates(jring, 1, Js, hdr, rows, max_n, t, n, mode, None)

    def release(t, n=1, jring=p, hdr=p, rows=1, max_out=most, ring=p, ring_len=8, Js=64):
        return l.afx_k_jitter_release_rates(jring, 1, Js, hdr, rows, t, n, max_out, ring, ring_len, None)

    good, keep = table()
    # refused on the host with nothing launched (there is no GPU here to launch on), each with its entry point's name
    cases = [
        (place, dict(n=0), b"1 to 16 rates"), (place, dict(n=17), b"1 to 16 rates"), (place, dict(t=None), b"null rate table"),
        (place, dict(stage=None), b"null"), (place, dict(hdr=None), b"null"), (place, dict(jring=None), b"null"),
        (place, dict(rows=0), b"rows"), (place, dict(rows=65536), b"rows"), (place, dict(max_n=65), b"fit"),
        (place, dict(Js=63), b"1 <= J <= Js"), (place, dict(t=table(J=0)), b"1 <= J <= Js"), (place, dict(t=table(L=0)), b"bad filter shape"),
        (place, dict(t=table(taps=None)), b"identity"), (place, dict(t=table(T=66)), b"history"),
        (conceal, dict(n=0), b"1 to 16 rates"), (conceal, dict(mode=2), b"mode"), (conceal, dict(t=table(fade=None)), b"fade"),
        (conceal, dict(t=table(P=0)), b"fade"), (conceal, dict(t=table(F=-1)), b"fade"), (conceal, dict(jring=None), b"null"),
        (conceal, dict(hdr=None), b"null"), (conceal, dict(rows=0), b"rows"), (conceal, dict(max_n=65), b"fit"),
        (conceal, dict(t=table(J=65)), b"1 <= J <= Js"), (conceal, dict(t=table(M=0)), b"bad filter shape"),
        (release, dict(n=17), b"1 to 16 rates"), (release, dict(t=None), b"null rate table"), (release, dict(max_out=None), b"null output counts"),
        (release, dict(jring=None), b"null"), (release, dict(hdr=None), b"null"), (release, dict(ring=None), b"null"),
        (release, dict(rows=0), b"rows"), (release, dict(ring_len=0), b"fit"),
        (release, dict(max_out=(ctypes.c_int * 16)(*([9] * 16))), b"fit"),  # beyond ring_len
        (release, dict(t=table(T=0)), b"bad filter shape"), (release, dict(t=table(T=66)), b"history"), (release, dict(t=table(J=65)), b"1 <= J <= Js"),
        (release, dict(t=table(L=1, M=16, T=20)), b"ratio above 12"), (release, dict(t=table(taps=None, L=1, M=2, T=1)), b"identity"),
    ]
    for fn, kw, text in cases:
        kw = dict(kw)
        t = kw.pop("t", good)
        t = t[0] if isinstance(t, tuple) else t
        assert fn(t, **kw) != 0
        err = l.afx_last_error()
        assert text in err and ("jitter_%s_rates" % fn.__name__).encode() in err, (fn.__name__, kw, err)
    # the second of two rates is checked like the first
    two, arr = table(2)
    arr[1].J = 65
    assert release(two, n=2) != 0 and b"1 <= J <= Js" in l.afx_last_error()
    # nothing to do is not an error, and launches nothing: a place / conceal of no samples, a release of no outputs
    zero = (ctypes.c_int * 16)()
    assert place(good, max_n=0) == 0 and conceal(good, max_n=0) == 0 and release(good, max_out=zero) == 0
    assert conceal(table(fade=None, P=0, F=0)[0], max_n=0, mode=0) == 0  # mode 0 reads no fade, period or fade length
