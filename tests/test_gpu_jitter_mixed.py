"""Every slot its own clock rate in one jitter buffer, on the GPU (afx/jitter.py MixedJitterScorer, afx_k_jitter_place_rates /
_conceal_rates / _release_rates).  The references are what this change leaves alone: the numpy statement of the played-out
stream E (oracle/jitter.py) with the offline ``Resampler`` over it (and float64 upfirdn), and the one-rate ``JitterScorer`` fed a slot's own
packets in the same calls.  Every comparison is exact but the float64 one, whose bound is tests/test_gpu_jitter.py's.
The one-rate and the ``_rates`` entry points are one kernel per verb behind two wrappers; the last test drives all seven
directly against oracle/jitter.py's ``NumpyDevice``."""
import random

import numpy as np
import pytest
import torch

from oracle.jitter import NumpyDevice, RefSlot, Schedule as _Schedule, packet as _packet, per_packet, rtp, sizing
from packet_helpers import offline as _offline, ref64 as _ref64, tap as _tap

pytestmark = pytest.mark.gpu

H = 4000
FORMATS = [(8000, "mulaw"), (8000, "alaw"), (11025, "pcm_s16le"), (16000, "pcm_f32le"), (48000, "pcm_s16le")]
ENC_AT = {8000: ("mulaw", "alaw"), 11025: ("pcm_s16le",), 16000: ("pcm_f32le",), 48000: ("pcm_s16le",)}
DEPTH_MS = 60


def _sizing(rate, mode):
    return sizing(rate, mode, DEPTH_MS, H)


def Schedule(rate, encodings, seed, jump=0, P=0, quiet=False, **kw):
    return _Schedule(rate, encodings, seed, jump=jump, short=max(1, P // 2), payload=per_packet(quiet=quiet), **kw)


def _rows_of(ticks, rng):
    """{slot: its tick} -> the rows of one feed: the slots' rows interleaved, each slot's own rows in their order of arrival."""
    order = [s for s, r in ticks.items() for _ in r]
    rng.shuffle(order)
    its = {s: iter(r) for s, r in ticks.items()}
    return [(s,) + next(its[s]) for s in order]


SLOT_RATES = [8000, 8000, 11025, 16000, 48000, 11025]  # slot 0 alternates mu-law and A-law per packet


@pytest.mark.parametrize("mode", ["repeat", "zero"])
def test_played_out_stream_of_every_rate_is_the_offline_resampling_of_the_numpy_stream(mode):
    from afx.jitter import MixedJitterScorer
    from afx.resample import Resampler
    S = 6
    tap = _tap(S)
    ms = MixedJitterScorer(tap, FORMATS, DEPTH_MS, conceal=mode, max_pending=3)
    ms.reset(list(range(S)), SLOT_RATES)
    # the tap placements this test is about: LDS taps, taps from global memory, the identity, M / L = 3
    shape = {r: Resampler(r) for r in set(SLOT_RATES)}
    assert shape[8000].L * (shape[8000].T | 1) <= 12288 < shape[11025].L * (shape[11025].T | 1) and shape[16000].identity
    assert (shape[48000].L, shape[48000].M) == (1, 3)
    geo = [_sizing(r, mode) for r in SLOT_RATES]
    depth, P, F, J = ([g[i] for g in geo] for i in (0, 1, 2, 5))
    assert (ms.rates.tolist(), ms.depths.tolist(), ms.periods.tolist(), ms.fades.tolist()) == (SLOT_RATES, depth, P, F)
    assert ms.Js == max(J) and tuple(ms.jring.shape) == (S, ms.Js) and len(set(J)) == 4
    # columns at and beyond a slot's own J: a NaN pattern that must come through the run bit for bit
    sentinel = torch.full((S, ms.Js), float("nan"), device="cuda").view(torch.int32) + torch.arange(ms.Js, device="cuda", dtype=torch.int32)
    for s in range(S):
        ms.jring[s, J[s]:] = sentinel.view(torch.float32)[s, J[s]:]
    assert torch.isnan(ms.jring[0, J[0]:]).all() and not ms.jring[:, :min(J)].any()
    seed = 77 + (7 if mode == "zero" else 0)
    rng = random.Random(seed)
    Pn = [r // 100 for r in SLOT_RATES]  # the traffic is made for the 10-ms period and its 30-ms fade in either mode
    Fn = [3 * p for p in Pn]
    sch = [Schedule(r, ENC_AT[r] if s == 0 or r != 8000 else ("alaw",), seed + 1000 * s, jump=J[s] + 123 + s, P=Pn[s],
                    origin=(1 << 32) - 3000 if s in (0, 4) else None) for s, r in enumerate(SLOT_RATES)]
    assert set(sch[0].enc) == {"mulaw", "alaw"}
    refs = [RefSlot(depth[s], mode, P[s], F[s]) for s in range(S)]
    L, M = [shape[r].L for r in SLOT_RATES], [shape[r].M for r in SLOT_RATES]
    hops = [0] * S
    while not all(sc.done() for sc in sch):
        ticks = {s: sch[s].tick() for s in range(S) if not sch[s].done() and rng.random() < 0.8}
        if not ticks:
            continue
        rows = _rows_of(ticks, rng)
        named = []
        for s, ts, t, raw, x, e in rows:
            refs[s].packet(t, x)
            named += [s] if s not in named else []
        for s in named:
            refs[s].after_feed()
        made = {s: -(-refs[s].next * L[s] // M[s]) for s in named}
        score = rng.random() < 0.6 or any(made[s] - hops[s] * H > 3 * H for s in named)
        res = ms.feed([r[3] for r in rows], [r[0] for r in rows], [r[1] for r in rows], score=score, encodings=[r[5] for r in rows])
        assert res.counts.shape == (len(rows),) and res.scores.shape == (int(res.counts.sum()),)
        for s in named:
            if score:  # every hop whose last input sample has been released is out, in this call
                assert len(tap.got[s]) == made[s] // H and int(ms.pending[s]) == made[s] % H
            assert int(ms.pending[s]) + H * len(tap.got[s]) == made[s] and int(ms.samples_in[s]) == refs[s].next
            assert int(ms.buffered[s]) == refs[s].hi - refs[s].next <= depth[s]
            hops[s] = len(tap.got[s])
    ms.flush()
    st = ms.stats()
    for s, rate in enumerate(SLOT_RATES):
        r = refs[s]
        r.release(r.hi)
        assert int(ms.samples_in[s]) == r.next == r.hi and int(ms.buffered[s]) == 0
        assert (int(st["received"][s]), int(st["late"][s]), int(st["duplicate"][s]), int(st["concealed"][s])) == \
            tuple(r.stats[k] for k in ("received", "late", "duplicate", "concealed"))
        # the traffic: two gaps closer than P in one release, a gap beyond the fade, a jump beyond the slot's own J
        assert any(len(g) >= 2 and any(b[0] - a[1] < Pn[s] for a, b in zip(g, g[1:])) for g in r.releases)
        lens = [e - a for a, e in r.spans]
        assert max(lens) > J[s] and sum(1 for n in lens if Fn[s] + Pn[s] < n < J[s]) >= 1 and r.stats["duplicate"] > 0 and len(sch[s].lost) >= 6
        E = np.array(r.E, dtype=np.float32)
        whole = _offline(E, rate)
        n_h = whole.numel() // H
        assert len(tap.got[s]) == n_h >= 6 and int(ms.pending[s]) == whole.numel() - n_h * H
        got = torch.cat(tap.got[s])
        assert torch.equal(got, whole[: n_h * H]), (rate, mode, s)
        assert np.abs(got.cpu().double().numpy() - _ref64(E, rate)[: n_h * H]).max() <= 2e-6 * float(np.abs(E).max())
        ex = ms.export_slots([s])
        k = int(ex.tensors["jitter_fill"][0])
        assert torch.equal(ex.tensors["jitter_pending"][0, :k], whole[n_h * H:]) and not ex.tensors["jitter_pending"][0, k:].any()
        # the slot wrapped its ring at its own J and never touched a column at or beyond it
        assert r.next > 2 * J[s] and torch.equal(ms.jring[s, J[s]:].view(torch.int32), sentinel[s, J[s]:])


def test_a_feed_of_every_rate_is_one_place_and_one_release_call_per_round(monkeypatch):
    from afx._lib import lib
    from afx.jitter import MixedJitterScorer
    S = 6
    tap = _tap(S)
    ms = MixedJitterScorer(tap, FORMATS, DEPTH_MS)
    ms.reset(list(range(S)), SLOT_RATES)
    l = lib()
    names = ("afx_k_jitter_place_rates", "afx_k_jitter_conceal_rates", "afx_k_jitter_release_rates", "afx_k_jitter_place",
             "afx_k_jitter_place_mixed", "afx_k_jitter_conceal", "afx_k_jitter_release", "afx_k_ingest_pop")
    calls = {n: 0 for n in names}
    for name in names:
        real = getattr(l, name)

        def counted(*args, _real=real, _name=name):
            calls[_name] += 1
            return _real(*args)

        monkeypatch.setattr(l, name, counted)
    g = np.random.default_rng(3)
    encs = ["mulaw", "alaw", "pcm_s16le", "pcm_f32le", "pcm_s16le", "pcm_s16le"]
    order = [4, 0, 5, 2, 1, 3]
    t = 0
    per_feed = []
    data = [[] for _ in range(S)]
    for k in range(8):  # 160 ms of in-order audio per slot: one round per feed, a release from the fourth feed on
        before = dict(calls)
        pk = {s: _packet(encs[s], SLOT_RATES[s] // 50, g) for s in order}
        for s in order:
            data[s].append(pk[s][1])
        res = ms.feed([pk[s][0] for s in order], order, [k * (SLOT_RATES[s] // 50) for s in order], encodings=[encs[s] for s in order])
        per_feed.append({n: calls[n] - before[n] for n in names})
        assert int(res.counts.sum()) == 0
    for k, c in enumerate(per_feed):  # whatever the number of rates: one place and at most one release, no one-rate entry point
        assert c["afx_k_jitter_place_rates"] == 1 and c["afx_k_jitter_release_rates"] == (1 if k >= 3 else 0), (k, c)
        assert not any(c[n] for n in names[3:7]) and c["afx_k_jitter_conceal_rates"] == 0
    monkeypatch.undo()
    ms.flush()
    for s, rate in enumerate(SLOT_RATES):  # and it computed the right thing
        whole = _offline(np.concatenate(data[s]), rate)
        k = int(ms.pending[s])
        assert k == whole.numel() and torch.equal(ms.export_slots([s]).tensors["jitter_pending"][0, :k], whole)


# ---- over the real scorers -------------------------------------------------------------------------------------------------
_ENGINE = []


def _inner(kind, S):
    from afx import engine, synth
    from afx.streaming import IncrementalScorer, KVCachedScorer
    if not _ENGINE:
        sd = synth.model_state_dict("ConformerModel", n_layers=1, n_encoders=1)
        eng = engine.Engine("conformer", n_layers=1, dtype="fp16", conf_blocks=1)
        eng.load_state_dict(sd)
        _ENGINE.append((eng, sd))
    eng, sd = _ENGINE[0]
    if kind == "incremental":
        return IncrementalScorer(eng, sd, S, window=16000, hop=H)
    return KVCachedScorer(eng, sd, S, window=64000, hop=H)


def _one_rate(kind, rate, mode):
    """The scorer of the contract for a slot at ``rate``: a JitterScorer of that rate over a same-weights inner scorer."""
    from afx.jitter import JitterScorer
    depth, P, F, _, _, _ = _sizing(rate, mode)
    kw = dict(period=P, fade=F) if mode == "repeat" else {}
    return JitterScorer(_inner(kind, 1), rate, ENC_AT[rate], depth, conceal=mode, **kw)


def _by_slot(res, slots):
    """A FeedResult over the rows ``slots`` -> {slot: (its scores, its hop count)}."""
    out = {}
    for s, part in zip(slots, res.split()):
        out.setdefault(s, []).append(part)
    return {s: (torch.cat(p), sum(x.numel() for x in p)) for s, p in out.items()}


@pytest.mark.parametrize("kind,mode", [("incremental", "repeat"), ("kv", "zero")])
def test_mixed_scores_stats_and_counts_equal_the_one_rate_jitter_scorers(kind, mode):
    from afx.jitter import MixedJitterScorer
    S = 6
    rates = list(SLOT_RATES)
    ms = MixedJitterScorer(_inner(kind, S), FORMATS, DEPTH_MS, conceal=mode)
    ms.reset(list(range(S)), rates)
    refs = [_one_rate(kind, r, mode) for r in rates]  # slot s's reference, fed slot s's packets alone (as its slot 0)
    rng = random.Random(11 + len(kind))
    new = lambda s, seed: Schedule(rates[s], ENC_AT[rates[s]] if s == 0 or rates[s] != 8000 else ("alaw",), seed,
                                   jump=_sizing(rates[s], mode)[5] + 50 if s == 2 else 0, P=rates[s] // 100, quiet=True)
    sch = [new(s, 500 + s) for s in range(S)]
    emitted, calls, buffered, changed = [0] * S, 0, 0, False
    while not all(sc.done() for sc in sch):
        calls += 1
        if calls == 25:  # slot 4 (48 kHz) ends its call and starts an 8 kHz one; its neighbours go on
            ms.reset([4], 8000)
            rates[4], changed = 8000, True
            refs[4] = _one_rate(kind, 8000, mode)
            sch[4] = new(4, 900)
            assert ms.rates.tolist() == rates and int(ms.samples_in[4]) == 0 and int(ms.pending[4]) == 0
        ticks = {s: sch[s].tick() for s in range(S) if not sch[s].done() and rng.random() < 0.8}
        if not ticks:
            continue
        rows = _rows_of(ticks, rng)
        slots = [r[0] for r in rows]
        fits = all(int(ms.pending[s]) + 2 * (int(ms.buffered[s]) + sum(len(r[4]) for r in rows if r[0] == s)) + 2 <= 4 * H for s in ticks)
        score = not (calls % 4 == 2 and fits)
        buffered += not score
        got = _by_slot(ms.feed([r[3] for r in rows], slots, [r[1] for r in rows], score=score, encodings=[r[5] for r in rows]), slots)
        for s in ticks:
            mine = [r for r in rows if r[0] == s]
            want = refs[s].feed([r[3] for r in mine], [0] * len(mine), [r[1] for r in mine], score=score, encodings=[r[5] for r in mine])
            assert got[s][1] == int(want.counts.sum()) and torch.equal(got[s][0], want.scores), (kind, s, calls)
            emitted[s] += got[s][1]
        if calls % 4 == 3:  # what the buffered feed before this one left comes out of a drain, slot by slot as in the reference
            res = ms.drain()
            for s, part in enumerate(res.split()):
                assert torch.equal(part, refs[s].drain([0]).scores), (kind, s, calls)
                emitted[s] += part.numel()
        for s in range(S):
            a, b = ms.stats(), refs[s].stats()
            assert all(int(a[k][s]) == int(b[k][0]) for k in a), (s, calls)
            assert (int(ms.samples_in[s]), int(ms.buffered[s]), int(ms.pending[s])) == \
                (int(refs[s].samples_in[0]), int(refs[s].buffered[0]), int(refs[s].pending[0]))
    res = ms.flush()
    for s, part in enumerate(res.split()):
        assert torch.equal(part, refs[s].flush([0]).scores)
        emitted[s] += part.numel()
    assert changed and buffered >= 3 and all(e >= 3 for e in emitted) and int(ms.stats()["concealed"].min()) > 0
    assert ms.samples_seen.tolist() == [int(refs[s].samples_seen[0]) for s in range(S)]


def _gapped(rate, encoding, seed, n_pk=40, lost=(10, 11, 24)):
    """In-order 20-ms packets of one stream with a few lost -> [(timestamp, bytes)]; after packet 13 has been fed with a depth
    of three packets the playout point stands inside the gap of packets 10 and 11."""
    g = np.random.default_rng(seed)
    n = rate // 50
    return [((seed * 7919 + k * n) % (1 << 32), _packet(encoding, n, g, quiet=True)[0]) for k in range(n_pk) if k not in lost]


def test_sessions_move_mid_gap_between_mixed_scorers_and_in_from_a_plain_jitter_scorer():
    from afx.jitter import JitterScorer, MixedJitterScorer
    from afx.streaming import StreamState
    kind = "incremental"
    A = MixedJitterScorer(_inner(kind, 3), [(8000, "mulaw"), (48000, "pcm_s16le"), (16000, "pcm_s16le")], DEPTH_MS)
    A.reset([0, 1], [8000, 48000])
    B = MixedJitterScorer(_inner(kind, 3), [(48000, "pcm_s16le"), (16000, "pcm_f32le"), (8000, "alaw"), (8000, "mulaw")], DEPTH_MS,
                          max_pending=3)
    P = JitterScorer(_inner(kind, 2), 48000, "pcm_s16le", DEPTH_MS * 48)  # (its default period and fade are the mixed scorer's)
    streams = [_gapped(8000, "mulaw", 1), _gapped(48000, "pcm_s16le", 2), _gapped(48000, "pcm_s16le", 3)]
    src = [(A, 0), (A, 1), (P, 1)]
    for k in range(12):  # packets 0..9, 12 and 13: hi is 14 packets, the playout point 11 packets, in the gap that began at 10
        for (sc, s), st in zip(src, streams):
            sc.feed([st[k][1]], [s], [st[k][0]])
    for (sc, s), r in zip(src, (8000, 48000, 48000)):
        book = sc.export_slots([s]).tensors["jitter_book"][0].tolist()
        assert book[2:5] == [11 * (r // 50), 14 * (r // 50), 10 * (r // 50)]
    st = A.export_slots([1, 0])
    assert st.tensors["jitter_rate"].tolist() == [48000, 8000] and st.tensors["jitter_params"].tolist() == [[2880, 480, 1440], [480, 80, 240]]
    own = 80 + 240 + 480
    assert tuple(st.tensors["jitter_ring"].shape) == (2, 480 + 1440 + 2880) and st.tensors["jitter_ring"][1, :own].any()
    assert not st.tensors["jitter_ring"][1, own:].any() and "input_rate" not in st.meta and st.meta["jitter_mixed"] == 1
    B.import_slots([2, 0], StreamState.from_state_dict(st.to("cpu").state_dict()))
    B.import_slots([1], P.export_slots([1]).to("cpu"))
    assert B.rates.tolist() == [8000, 48000, 48000] and B.samples_in.tolist() == [11 * 160, 11 * 960, 11 * 960]
    moved = {0: 0, 2: 1, 1: 2}  # B's slot -> the stream (and its unmoved source)
    scores = 0
    for k in range(12, len(streams[0])):
        named = [2, 0, 1] if k % 2 else [1, 2, 0]
        res = B.feed([streams[moved[b]][k][1] for b in named], named, [streams[moved[b]][k][0] for b in named],
                     encodings=["mulaw" if moved[b] == 0 else "pcm_s16le" for b in named])  # (B's default at 8 kHz is A-law)
        for b, part in zip(named, res.split()):
            sc, s = src[moved[b]]
            assert torch.equal(part, sc.feed([streams[moved[b]][k][1]], [s], [streams[moved[b]][k][0]]).scores), (b, k)
            scores += part.numel()
    res = B.flush([0, 2, 1])
    for b, part in zip([0, 2, 1], res.split()):
        sc, s = src[moved[b]]
        assert torch.equal(part, sc.flush([s]).scores)
        scores += part.numel()
        assert {k: int(v[b]) for k, v in B.stats().items()} == {k: int(v[s]) for k, v in sc.stats().items()}
    assert scores >= 6 and int(B.stats()["concealed"].min()) == 3 * 160


def _rtp(seq, ts, pt, payload, ssrc):
    return rtp(seq & 0xFFFF, ts & 0xFFFFFFFF, pt=pt, ssrc=ssrc, payload=payload)  # (the callers' counters run past the wrap)


def test_feed_rtp_with_static_and_dynamic_payload_types_equals_feed():
    from afx.jitter import MixedJitterScorer
    formats = [(8000, "mulaw"), (8000, "alaw"), (16000, "pcm_s16le")]
    ta, tb = _tap(2), _tap(2)
    a, b = MixedJitterScorer(ta, formats, DEPTH_MS), MixedJitterScorer(tb, formats, DEPTH_MS)
    for m in (a, b):
        m.reset([1], 16000)
    g = np.random.default_rng(4)
    order = [k for k in range(60) if k not in (7, 20, 21)]
    order[30], order[32], order[40], order[41] = order[32], order[30], order[41], order[40]
    types = {96: (16000, "pcm_s16le")}
    for k in order:
        pt = 0 if k % 2 else 8
        enc = ["mulaw" if pt == 0 else "alaw", "pcm_s16le"]
        pay = [_packet(enc[0], 160, g)[0], _packet(enc[1], 320, g)[0]]
        ts = [((1 << 32) - 1000 + k * 160) % (1 << 32), (77 + k * 320) % (1 << 32)]
        a.feed_rtp([_rtp(65530 + k, ts[1], 96, pay[1], 0xB), _rtp(65530 + k, ts[0], pt, pay[0], 0xA)], [1, 0], payload_types=types)
        b.feed([pay[1], pay[0]], [1, 0], [ts[1], ts[0]], encodings=[enc[1], enc[0]])
    with pytest.raises(ValueError):
        a.feed_rtp([_rtp(1, 0, 0, bytes(160), 0xB)], [1], payload_types=types)  # PT 0 is 8 kHz, slot 1 is at 16 kHz
    a.flush()
    b.flush()
    for s in (0, 1):
        assert len(ta.got[s]) == len(tb.got[s]) >= 4 and torch.equal(torch.cat(ta.got[s]), torch.cat(tb.got[s]))
    assert a.stats()["concealed"].tolist() == [3 * 160, 3 * 320] == b.stats()["concealed"].tolist()
    assert a.stats()["out_of_order"].tolist() == b.stats()["out_of_order"].tolist() and min(a.stats()["out_of_order"].tolist()) >= 2


def test_one_rate_entry_points_are_the_rates_kernels_with_a_table_of_one_entry():
    """The seven entry points driven directly.  Each verb runs through its one-rate entry point and, on a clone of the
    buffers, through its ``_rates`` entry point with a table of two rates in which the rate under test is entry 1: the
    whole buffers must come out bit-equal, sentinels included.  Place and conceal must equal oracle/jitter.py's
    ``NumpyDevice`` bit for bit; release the float64 sum over the same fp32 taps within the bound of the
    float64 comparison above (2e-6 of the largest input).  The rows wrap the ring column and ``wpos``, one has n = 0, one names
    slot S and must be skipped whole; the three rates take the copy, the LDS-tap and the global-tap path of the release."""
    import ctypes as C
    from types import SimpleNamespace

    from afx._lib import JitterRate, call_on, check, lib, ptr
    from afx.ingest import ENCODINGS, layout, plan as ingest_plan
    from afx.resample import Resampler
    packet_of = lambda e, n, g: _packet(e, n, g, amp=1.0, div=1)  # full-scale noise
    l, S, hop, P, F = lib(), 3, 512, 8, 16
    R = 2 * hop  # the pending ring
    rs = {r: Resampler(r) for r in (16000, 8000, 11025)}
    path = {r: "copy" if x.identity else "lds" if x.L * (x.T | 1) <= 12288 else "global" for r, x in rs.items()}  # poly_grid's rule
    assert sorted(path.values()) == ["copy", "global", "lds"], path
    bits = lambda t: t.view(torch.int32)
    fade_of = lambda n: torch.from_numpy((1.0 - np.arange(max(n, 1), dtype=np.float64) / max(n, 1)).astype(np.float32)).cuda()
    sentinel = lambda *shape: (torch.arange(int(np.prod(shape)), dtype=torch.int32) + 0x3C000000).view(torch.float32).reshape(shape)

    def both(one, rated, buf):
        a, b = buf.clone(), buf.clone()
        one(a)
        rated(b)
        torch.cuda.synchronize()
        assert torch.equal(bits(a), bits(b))
        return a

    for rate, x in rs.items():
        g = np.random.default_rng(rate)
        L, M, T = x.L, x.M, 1 if x.identity else x.T
        taps = None if x.identity else ptr(x.taps)
        J = max(T - 1, P + F) + -(-hop * M // L) + 1  # lookback + W at depth 0
        assert J >= 281 and J + 8 <= R
        # the table: entry 0 another rate with its own J, P, F and fade; entry 1 the rate under test; Js = J
        other, fades = rs[8000 if x.identity else 16000], [fade_of(8), fade_of(F)]
        table = (JitterRate * 2)()
        for t, y, geo, f in zip(table, (other, x), ((J - 7, 4, 8), (J, P, F)), fades):
            t.taps, t.fade = None if y.identity else y.taps.data_ptr(), f.data_ptr()
            t.L, t.M, t.T = y.L, y.M, 1 if y.identity else y.T
            t.J, t.P, t.F = geo
        tp = C.cast(table, C.c_void_p)
        host = SimpleNamespace(_rated=True, _mixed=True, jring=sentinel(S, J), _table=table, _fades=[f.cpu() for f in fades], S=S, ring_len=R,
                               _rate_of=np.ones(S, dtype=np.int64), conceal="repeat")
        ref = NumpyDevice(host)  # (its ring is host.jring's memory)
        jr = host.jring.clone().cuda()

        def upload(rows):
            return torch.from_numpy(np.array(rows, dtype=np.int32)).cuda()

        # ---- place: four encodings through place_mixed, then one launch of afx_k_jitter_place -------------------------------
        launches = [[(0, "mulaw", 40, J - 3), (1, "alaw", 0, 5), (2, "pcm_s16le", 270, 7), (S, "pcm_f32le", 20, 0)],
                    [(1, "pcm_f32le", 33, J - 3), (0, "alaw", 17, 50), (2, "mulaw", 0, 9)],
                    [(2, "pcm_s16le", 64, J - 3), (0, "pcm_s16le", 9, 0), (S, "pcm_s16le", 5, 1)]]
        for k, rows in enumerate(launches):
            pay = [packet_of(e, n, g)[0] for _, e, n, _ in rows]
            offs, total = layout([len(p) for p in pay])
            stage = np.zeros(total, dtype=np.uint8)
            for o, p in zip(offs, pay):
                stage[o:o + len(p)] = np.frombuffer(p, dtype=np.uint8)
            stage = torch.from_numpy(stage).cuda()
            r6 = [(s, o, n, c, ENCODINGS.index(e), 1) for (s, e, n, c), o in zip(rows, offs)]
            most = max(r[2] for r in r6)
            h6 = upload(r6)
            if k < 2:
                h, one = upload([r[:5] for r in r6]), lambda b: check(call_on(b, l.afx_k_jitter_place_mixed, ptr(stage), total, ptr(h), len(r6), most, ptr(b), S, J))
            else:
                h, one = upload([r[:4] for r in r6]), lambda b: check(call_on(b, l.afx_k_jitter_place, ptr(stage), total, ptr(h), len(r6), most, ENCODINGS.index("pcm_s16le"), ptr(b), S, J))
            jr = both(one, lambda b: check(call_on(b, l.afx_k_jitter_place_rates, ptr(stage), total, ptr(h6), len(r6), most, tp, 2, ptr(b), S, J)), jr)
            ref.run(SimpleNamespace(ops=[("place", np.array([r for r in r6 if r[0] < S and r[2] > 0], dtype=np.int32), most)]), pay)
            assert torch.equal(bits(jr.cpu()), bits(host.jring)), (rate, "place", k)
        # ---- conceal: repeat (a wrap, beyond the fade, n = 0, slot S), then zero over more than one block ------------------------
        for mode, rows in (("repeat", [(0, J - 3, 0, 40), (1, 30, 5, 5), (2, 20, 3, 10), (S, 0, 0, 5)]), ("zero", [(1, J - 3, 0, 260), (S, 4, 0, 9)])):
            host.conceal, m = mode, ("zero", "repeat").index(mode)
            most = max(hi - lo for _, _, lo, hi in rows)
            h4, h5 = upload(rows), upload([r + (1,) for r in rows])
            jr = both(lambda b: check(call_on(b, l.afx_k_jitter_conceal, ptr(b), S, J, ptr(h4), len(rows), most, ptr(fades[1]), P, F, m)),
                      lambda b: check(call_on(b, l.afx_k_jitter_conceal_rates, ptr(b), S, J, ptr(h5), len(rows), most, tp, 2, m)), jr)
            ref.run(SimpleNamespace(ops=[("conceal", np.array([r + (1,) for r in rows if r[0] < S and r[3] > r[2]], dtype=np.int32), most)]), [])
            assert torch.equal(bits(jr.cpu()), bits(host.jring)), (rate, "conceal", mode)
        # ---- release: the one-rate entry point does not read the eighth int, so both take the same rows --------------------------
        rows = [(s, N % J, n_in) + ingest_plan(N, n_in, L, M) + (wpos, 1)
                for s, N, n_in, wpos in ((0, 3 * J - 3, J - max(T - 1, P + F), R - 5), (1, J + 11, 0, 7), (2, 2 * J + 40, 100, 0), (S, 0, 10, 0))]
        most = max(r[3] for r in rows)
        assert rows[0][1] == J - 3 and 256 < most <= R and rows[1][3] == 0
        h8, counts = upload(rows), np.array([0, most], dtype=np.int32)
        ring0 = sentinel(S, R).cuda()
        ring = both(lambda b: check(call_on(b, l.afx_k_jitter_release, ptr(jr), S, J, ptr(h8), len(rows), most, taps, L, M, T, ptr(b), R)),
                    lambda b: check(call_on(b, l.afx_k_jitter_release_rates, ptr(jr), S, J, ptr(h8), len(rows), tp, 2,
                                            counts.ctypes.data_as(C.c_void_p), ptr(b), R)), ring0).cpu()
        assert torch.equal(bits(jr.cpu()), bits(host.jring))  # (only read)
        untouched = torch.ones(S, R, dtype=torch.bool)
        w64 = None if x.identity else x.taps.cpu().double().numpy()
        for s, col, n_in, n_out, p0, d0, wpos, _ in rows[:3]:
            v = host.jring[s].double().numpy()
            q = np.arange(n_out) * M + p0
            idx = (col + d0 + q // L)[:, None] - np.arange(T)[None, :]
            assert n_out == 0 or (idx.min() >= col - (T - 1) and idx.max() < col + n_in)
            want = v[idx[:, 0] % J] if x.identity else (w64[q % L] * v[idx % J]).sum(axis=1)
            at = (wpos + np.arange(n_out)) % R
            got = ring[s, at].double().numpy()
            tol = 0.0 if x.identity or not n_out else 2e-6 * float(np.abs(v[idx % J]).max())
            assert n_out == 0 or np.abs(got - want).max() <= tol, (rate, s, float(np.abs(got - want).max()), tol)
            untouched[s, at] = False
        assert not untouched[0, R - 5:].any() and not untouched[0, :5].any()  # (the wrap of wpos)
        assert torch.equal(bits(ring)[untouched], bits(ring0.cpu())[untouched]), (rate, "release")
