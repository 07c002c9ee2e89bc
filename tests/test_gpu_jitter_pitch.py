"""Pitch-period loss concealment on the GPU (afx/jitter.py conceal="pitch_sync"; afx_k_jitter_pitch / _conceal_period and their
_rates forms).  Every comparison is exact.  The estimate kernel alone against ``afx.jitter.pitch_reference`` (voiced signals,
noise, silence, an exact tie of scores, a history across the ring's wrap and one that begins in the zeros before the origin,
NaN / inf / out-of-range samples, rows that must write nothing); the synthesis kernel alone against its numpy statement (d
ranges across the hold, the fade's end and the ring's wrap, periods at both ends of the lags and a prime between, a stored
period outside the lags read as P0).  Then the played-out stream: the numpy reference (oracle/jitter.py's ``RefSlot``
at "pitch_sync"), under a network that loses, duplicates and shuffles packets, with two gaps closer than the search history in
one release, a gap longer than hold + fade, a gap released over three calls and a jump beyond the ring; a mixed-rate scorer
against the one-rate scorers; comfort noise after a mark; a session moved mid-gap through host memory; and one real model."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

from oracle.jitter import RefSlot, Schedule as _Schedule, coded as _stream, voiced, voiced_stream
from packet_helpers import offline as _offline, tap as _tap

pytestmark = pytest.mark.gpu

H = 4000
SENTINEL = np.float32(-7.25)


def Schedule(rate, encoding, seed, f0=None, **kw):
    return _Schedule(rate, encoding, seed, short=rate // 200, payload=voiced_stream(f0), **kw)  # 5 ms between two lost packets


def Ref(rate, depth, cn=None):
    return RefSlot(depth, "pitch_sync", rate=rate, noise=cn)


def bits(t):
    return t.contiguous().view(torch.int32)


def _params(rate):
    from afx.jitter import pitch_lags
    Pmin, Pmax, Wc = pitch_lags(rate)
    return Pmin, Pmax, Wc, rate // 100, rate // 100, rate // 20  # ..., P0, Hd, F


def _tables(rate, Js, entries):
    """The host tables of a ``_rates`` launch: entries of (J, gain tensor or None) at ``rate``'s parameters."""
    from afx._lib import JitterLags, JitterRate
    Pmin, Pmax, Wc, P0, Hd, F = _params(rate)
    rates, lags = (JitterRate * len(entries))(), (JitterLags * len(entries))()
    for r, g, (J, gain) in zip(rates, lags, entries):
        r.taps, r.fade, r.L, r.M, r.T, r.J, r.P, r.F = None, None if gain is None else gain.data_ptr(), 1, 1, 1, J, P0, F
        g.Pmin, g.Pmax, g.Wc, g.P0, g.Hd = Pmin, Pmax, Wc, P0, Hd
    return rates, lags


# ---- the estimate kernel alone -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [8000, 11025, 48000])
def test_the_estimate_kernel_writes_the_reference_period_of_every_row(rate):
    from afx._lib import call_on, check, lib, ptr
    from afx.jitter import pitch_reference
    Pmin, Pmax, Wc, P0, _, _ = _params(rate)
    Lh, l = Pmax + Wc, lib()
    S, J = 12, Pmax + Wc + 37
    g = np.random.default_rng(rate)
    tie = np.tile(g.integers(-9000, 9000, 40), Lh // 40 + 2)[:Lh].astype(np.float32) / np.float32(32768)  # exactly periodic: 40
    odd = voiced(rate, 125, Lh, 7)
    odd[[3, Lh - Wc + 5, Lh - 9, Lh - Wc - 11, Lh - 30]] = [np.nan, np.inf, -np.inf, 3.0, -2.5]
    short = np.concatenate([np.zeros(Lh - Wc - 33, np.float32), voiced(rate, 97, Wc + 33, 8)])  # begins before the origin: zeros
    cases = [(voiced(rate, 97, Lh, 1), J - 5), (voiced(rate, 180, Lh, 2), Lh), (0.1 * g.standard_normal(Lh).astype(np.float32), J - 1),
             (np.zeros(Lh, np.float32), Lh + 3), (tie, Lh + 1), (voiced(rate, 260, Lh, 3), Lh // 2), (short, 11), (odd, Wc)]
    if rate == 48000:  # one row is enough at this size: a voiced history across the wrap
        cases = cases[5:6]
    slots = [9, 0, 4, 2, 11, 7, 5, 1][:len(cases)]
    ring = np.full((S, J), SENTINEL, np.float32)
    rows, want = [], np.full(S, -77, np.int32)
    for (hist, ac), s in zip(cases, slots):
        ring[s, (ac - Lh + np.arange(Lh)) % J] = hist
        rows.append((s, ac))
        want[s] = pitch_reference(hist, rate)
    assert any(ac < Lh for _, ac in cases) and (rate == 48000 or any(ac >= Lh for _, ac in cases))
    if rate != 48000:
        assert want[2] == P0 and want[11] == 40 and Pmin <= want[9] <= Pmax and len(set(want[slots].tolist())) >= 4
    skipped = [(S, 5), (-1, 5), (3, J), (6, -1)]  # a slot or a column out of range: nothing is written
    jr = torch.from_numpy(ring).cuda()
    hdr = torch.tensor(rows + skipped, dtype=torch.int32).cuda()
    period = torch.full((S,), -77, dtype=torch.int32).cuda()
    check(call_on(jr, l.afx_k_jitter_pitch, ptr(jr), S, J, ptr(hdr), len(rows) + len(skipped), Pmin, Pmax, Wc, P0, ptr(period)))
    assert period.cpu().numpy().tolist() == want.tolist()
    assert torch.equal(bits(jr.cpu()), bits(torch.from_numpy(ring)))  # (only read)
    # the _rates form: rate 1 is the rate above; rate 0 has a ring one short of its history, so its rows write nothing
    rates, lags = _tables(rate, J, [(Lh - 1, None), (J, None)])
    hdr3 = torch.tensor([r + (1,) for r in rows + skipped] + [(3, 5, 0), (6, 5, 2), (8, 5, -1)], dtype=torch.int32).cuda()
    period2 = torch.full((S,), -77, dtype=torch.int32).cuda()
    check(call_on(jr, l.afx_k_jitter_pitch_rates, ptr(jr), S, J, ptr(hdr3), hdr3.shape[0], C.cast(rates, C.c_void_p),
                  C.cast(lags, C.c_void_p), 2, ptr(period2)))
    assert period2.cpu().numpy().tolist() == want.tolist()


# ---- the synthesis kernel alone ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [8000, 11025])
def test_the_synthesis_kernel_repeats_the_stored_period_under_hold_and_fade(rate):
    from afx._lib import call_on, check, lib, ptr
    from afx.jitter import gain_table
    Pmin, Pmax, Wc, P0, Hd, F = _params(rate)
    G, l = Hd + F, lib()
    prime = next(p for p in range((Pmin + Pmax) // 2, Pmax) if all(p % q for q in range(2, p)))
    S, J = 8, G + Pmax + 45
    g = np.random.default_rng(rate + 1)
    ring = (0.2 * g.standard_normal((S, J))).astype(np.float32)
    stored = np.array([Pmin, Pmax, prime, 0, Pmax + 1, Pmin - 1, prime, -5], dtype=np.int32)
    # slot, a mod J, d_lo, d_hi: across the hold and the wrap; across the hold and the fade's end over more than one block;
    # across the fade's end and the wrap; a source that wraps backwards; ...; the last: d_hi + Pmax > J, skipped whole
    rows = [(0, J - Hd // 2, 0, Hd + 20), (1, 300, Hd - 20, G + 20), (2, J - G - 3, G - 10, G + 10), (3, 5, 0, Hd + 10),
            (4, Pmax + 7, 3, 50), (5, J - 1, Hd, Hd + 77), (7, 9, 0, 0), (6, 20, 0, J - Pmax + 1)]
    assert rows[1][3] - rows[1][2] > 256 and rows[0][1] + rows[0][3] > J and rows[2][1] + rows[2][3] > J and rows[3][1] < Pmin
    gain = gain_table(Hd, F)
    assert gain.shape == (G,) and (gain[:Hd] == 1).all() and gain[Hd] == 1 and 0 < gain[-1] < gain[Hd + 1] < 1
    want = ring.copy()
    for s, ac, lo, hi in rows[:-1]:
        p = int(stored[s]) if Pmin <= stored[s] <= Pmax else P0
        d = np.arange(lo, hi)
        v = np.zeros(hi - lo, np.float32)
        m = d < G
        v[m] = gain[d[m]] * ring[s, (ac - p + d[m] % p) % J]
        want[s, (ac + d) % J] = v
    most = max(hi - lo for _, _, lo, hi in rows[:-1])
    gain_d, period = torch.from_numpy(gain).cuda(), torch.from_numpy(stored).cuda()
    a = torch.from_numpy(ring).cuda()
    hdr = torch.tensor(rows + [(S, 0, 0, 5)], dtype=torch.int32).cuda()
    check(call_on(a, l.afx_k_jitter_conceal_period, ptr(a), S, J, ptr(hdr), hdr.shape[0], most, ptr(gain_d), ptr(period), Pmin, Pmax,
                  P0, Hd, F))
    assert torch.equal(bits(a.cpu()), bits(torch.from_numpy(want)))  # (and every other column is unchanged)
    assert np.count_nonzero(want != ring) > sum(min(hi, G) - lo for _, _, lo, hi in rows[:5]) // 2
    assert period.cpu().numpy().tolist() == stored.tolist()
    # the _rates form writes the same bits; a row of a rate index out of range writes nothing
    rates, lags = _tables(rate, J, [(J, gain_d), (J - 1, gain_d)])
    b = torch.from_numpy(ring).cuda()
    hdr5 = torch.tensor([r + (0,) for r in rows] + [(7, 0, 0, 5, 2), (7, 0, 0, 5, -1)], dtype=torch.int32).cuda()
    check(call_on(b, l.afx_k_jitter_conceal_period_rates, ptr(b), S, J, ptr(hdr5), hdr5.shape[0], most, C.cast(rates, C.c_void_p),
                  C.cast(lags, C.c_void_p), 2, ptr(period)))
    assert torch.equal(bits(b.cpu()), bits(torch.from_numpy(want)))


def _rows(ticks, rng):
    """The rows of one feed from {slot: its tick}: the slots' rows interleaved, each slot's own in their order of arrival
    -> (rows of (slot, timestamp, index, bytes, decoded), the slots in the order first named)."""
    order = [s for s, r in ticks.items() for _ in r]
    rng.shuffle(order)
    its = {s: iter(r) for s, r in ticks.items()}
    rows = [(s,) + next(its[s]) for s in order]
    return rows, list(dict.fromkeys(r[0] for r in rows))


@pytest.mark.parametrize("encoding", ["mulaw", "pcm_f32le"])
@pytest.mark.parametrize("rate", [8000, 11025, 48000])
def test_played_out_stream_is_the_offline_resampling_of_the_numpy_stream(rate, encoding):
    from afx.jitter import JitterScorer
    S = 3
    depth = 3 * (rate // 50)  # 60 ms
    tap = _tap(S)
    js = JitterScorer(tap, rate, encoding, depth, conceal="pitch_sync", max_pending=3)
    Pmin, Pmax, Wc, P0, Hd, F = _params(rate)
    G, Lh = Hd + F, Pmax + Wc
    assert (js.period, js.fade_len, js.hold, js.lags, js.corr) == (P0, F, Hd, (Pmin, Pmax), Wc)
    seed = rate + 31 * len(encoding)
    rng = random.Random(seed)
    sch = [Schedule(rate, encoding, seed + 1000 * s, jump=js.J + 123 + s, origin=(1 << 32) - 3000 if s == 0 else None,
                    f0=(None, 125, None)[s]) for s in range(S)]
    refs = [Ref(rate, depth) for sc in sch]
    hops = [0] * S
    while not all(sc.done() for sc in sch):
        ticks = {s: sch[s].tick() for s in range(S) if not sch[s].done() and rng.random() < 0.8}
        if not ticks:
            continue
        rows, named = _rows(ticks, rng)
        for s, ts, t, raw, x, e in rows:
            refs[s].packet(t, x)
        for s in named:
            refs[s].after_feed()
        made = {s: -(-refs[s].next * js.L // js.M) for s in named}
        score = rng.random() < 0.6 or any(made[s] - hops[s] * H > 3 * H for s in named)
        res = js.feed([r[3] for r in rows], [r[0] for r in rows], [r[1] for r in rows], score=score)
        assert res.counts.shape == (len(rows),) and res.scores.shape == (int(res.counts.sum()),)
        for s in named:
            if score:  # every hop whose last input sample has been released is out, in this call
                assert len(tap.got[s]) == made[s] // H and int(js.pending[s]) == made[s] % H
            assert int(js.pending[s]) + H * len(tap.got[s]) == made[s] and int(js.samples_in[s]) == refs[s].next
            assert int(js.buffered[s]) == refs[s].hi - refs[s].next <= depth
            hops[s] = len(tap.got[s])
    js.flush()
    st = js.stats()
    for s in range(S):
        r = refs[s]
        r.release(r.hi)
        assert int(js.samples_in[s]) == r.next == r.hi and int(js.buffered[s]) == 0
        assert (int(st["received"][s]), int(st["late"][s]), int(st["duplicate"][s]), int(st["concealed"][s])) == \
            tuple(r.stats[k] for k in ("received", "late", "duplicate", "concealed"))
        # the traffic was what the issue asks for: two gaps closer than Lh in one release, a gap beyond hold + fade, a gap
        # released by at least three calls, a jump beyond J
        assert any(len(g) >= 2 and any(b[0] - a[1] < Lh for a, b in zip(g, g[1:])) for g in r.releases)
        lens = [e - a for a, e in r.spans]
        assert max(lens) > js.J and sum(1 for n in lens if G + Pmax < n < js.J) >= 1 and r.stats["duplicate"] > 0 and len(sch[s].lost) >= 6
        assert max(c for c, n in zip(r.calls, lens) if n < js.J) >= 3
        E = np.array(r.E, dtype=np.float32)
        a, e = next((a, e) for a, e in r.spans if a >= 10 * (rate // 50))  # concealed samples are there, and they are not zeros
        assert np.count_nonzero(E[a:min(e, a + G)]) > 0.8 * min(e - a, G) - 1
        if s == 1:  # the voiced slot, after Lh received samples: the search found the pitch (a multiple of rate / 125)
            found = [p for p, (a, _) in zip(r.periods, r.spans) if a > Lh and set(r.kinds[a - Lh:a]) == {"r"}]
            assert found and all(abs(p / (rate / 125) - round(p / (rate / 125))) * (rate / 125) <= 1 for p in found)
        whole = _offline(E, rate)
        n_h = whole.numel() // H
        assert len(tap.got[s]) == n_h >= 6 and int(js.pending[s]) == whole.numel() - n_h * H
        got = torch.cat(tap.got[s])
        assert torch.equal(got, whole[: n_h * H]), (rate, encoding, s)
        ex = js.export_slots([s])
        k = int(ex.tensors["jitter_fill"][0])
        assert torch.equal(ex.tensors["jitter_pending"][0, :k], whole[n_h * H:]) and not ex.tensors["jitter_pending"][0, k:].any()


# ---- mixed rates -------------------------------------------------------------------------------------------------------------------
def test_a_mixed_scorer_equals_the_one_rate_scorer_of_each_slot():
    from afx.jitter import JitterScorer, MixedJitterScorer
    formats = [(8000, "mulaw"), (16000, "pcm_s16le"), (48000, "pcm_f32le")]
    S, rng = 3, random.Random(5)
    tm = _tap(S)
    ms = MixedJitterScorer(tm, formats, 60, conceal="pitch_sync")
    ms.reset([0, 1, 2], [8000, 16000, 48000])
    taps = [_tap(S) for _ in range(S)]
    ones = [JitterScorer(taps[s], r, e, 60 * r // 1000, conceal="pitch_sync") for s, (r, e) in enumerate(formats)]
    assert ms.periods.tolist() == [o.period for o in ones] and ms.fades.tolist() == [o.fade_len for o in ones]
    sch = [Schedule(r, e, 77 + s, jump=ones[s].J + 9, f0=(180, None, 97)[s], n_pk=60) for s, (r, e) in enumerate(formats)]
    while not all(sc.done() for sc in sch):
        ticks = {s: sch[s].tick() for s in range(S) if not sch[s].done() and rng.random() < 0.8}
        if not ticks:
            continue
        rows, named = _rows(ticks, rng)
        res = ms.feed([r[3] for r in rows], [r[0] for r in rows], [r[1] for r in rows])
        for s in named:
            mine = [i for i, r in enumerate(rows) if r[0] == s]
            one = ones[s].feed([rows[i][3] for i in mine], [s] * len(mine), [rows[i][1] for i in mine])
            assert res.counts[mine].tolist() == one.counts.tolist()
    ms.flush()
    stm = ms.stats()
    for s in range(S):
        ones[s].flush([s])
        st = ones[s].stats()
        assert all(int(stm[k][s]) == int(st[k][s]) for k in st) and int(st["concealed"][s]) > ones[s].hold + ones[s].fade_len
        assert len(tm.got[s]) == len(taps[s].got[s]) >= 4 and torch.equal(bits(torch.cat(tm.got[s])), bits(torch.cat(taps[s].got[s])))
        a, b = ms.export_slots([s]), ones[s].export_slots([s])
        assert torch.equal(a.tensors["jitter_pitch"], b.tensors["jitter_pitch"])
        assert torch.equal(a.tensors["jitter_pending"], b.tensors["jitter_pending"])
    assert torch.equal(ms.jperiod.cpu(), torch.stack([ones[s].jperiod[s] for s in range(S)]).cpu())


# ---- comfort noise -----------------------------------------------------------------------------------------------------------------
def test_a_gap_with_a_mark_is_concealed_by_the_new_rule_before_it_and_noise_after():
    from afx.jitter import ComfortNoise, JitterScorer
    rate, S, n = 16000, 2, 320  # (16 kHz: the popped stream is E itself)
    cn = ComfortNoise(1234)
    tap = _tap(S)
    js = JitterScorer(tap, rate, "pcm_f32le", 3 * n, conceal="pitch_sync", comfort_noise=cn)
    x = voiced(rate, 180, 60 * n, 3)
    ref = Ref(rate, 3 * n, cn)
    mark = 11 * n + 7
    lost = {10, 11, 12, 13, 30, 31}
    for k in range(60):
        if k in lost:
            continue
        if k == 14:
            js.silence([1], [mark], [40])
            ref.mark(mark, 40)
        js.feed([x[k * n:(k + 1) * n].tobytes()], [1], [k * n])
        ref.packet(k * n, x[k * n:(k + 1) * n])
        ref.after_feed()
    js.flush([1])
    ref.release(ref.hi)
    st = js.stats()
    assert (int(st["concealed"][1]), int(st["comfort"][1])) == (ref.stats["concealed"], ref.stats["comfort"]) == (n + 7 + 2 * n, 3 * n - 7)
    E = np.array(ref.E, dtype=np.float32)
    assert ref.periods[0] != ref.P0 and np.count_nonzero(E[10 * n:mark]) > n  # the loss part: the voiced period, repeated
    assert np.array_equal(E[mark:14 * n], cn.samples(mark, 14 * n - mark, 40))
    got = torch.cat(tap.got[1])
    assert got.numel() == len(E) // H * H >= 4 * H and torch.equal(bits(got.cpu()), bits(torch.from_numpy(E[:got.numel()].copy())))


# ---- sessions ------------------------------------------------------------------------------------------------------------------------
def test_a_session_moved_mid_gap_through_host_memory_continues_bit_for_bit():
    from afx.jitter import JitterScorer
    rate, n = 8000, 160
    depth = 3 * n
    ta, tb, tc = _tap(2), _tap(2), _tap(3)
    A, B, Cc = (JitterScorer(t, rate, "mulaw", depth, conceal="pitch_sync") for t in (ta, tb, tc))
    raw, x = _stream("mulaw", 70 * n, 21, f0=97, rate=rate)
    ref = Ref(rate, depth)
    lost = {20, 21, 22, 23, 40}
    moved = None
    for k in range(70):
        if k in lost:
            continue
        pk, ts = raw[k * n:(k + 1) * n], 5000 + k * n
        A.feed([pk], [1], [ts])
        ref.packet(k * n, x[k * n:(k + 1) * n])
        ref.after_feed()
        if moved is None:
            B.feed([pk], [1], [ts])
        else:
            Cc.feed([pk], [0], [ts])
        if k == 24:  # the playout point stands 40 ms into the gap of 20..23: 0 < d < hold + fade
            assert ref.gap == 20 * n and 0 < ref.next - ref.gap < ref.G
            st = B.export_slots([1])
            assert st.meta["jitter_conceal"] == "pitch_sync" and st.meta["jitter_hold"] == B.hold
            assert st.meta["jitter_lags"] == B.lags + (B.corr,)
            assert st.tensors["jitter_pitch"].is_cuda and st.tensors["jitter_pitch"].tolist() == [ref.p] and ref.p != ref.P0
            host = st.to("cpu")
            assert not any(t.is_cuda for t in host.tensors.values())
            moved = len(tb.got[1])
            Cc.import_slots([0], host)
            assert Cc.jperiod.tolist() == [ref.p, 0, 0]
            B.reset([1])
            assert B.jperiod.tolist() == [0, 0]
    A.flush([1])
    Cc.flush([0])
    ref.release(ref.hi)
    whole = _offline(ref.E, rate)
    got = torch.cat(ta.got[1])
    assert moved is not None and len(tc.got[0]) >= 3 and torch.equal(bits(got), bits(whole[:got.numel()]))
    assert torch.equal(bits(torch.cat(tb.got[1][:moved] + tc.got[0])), bits(got))
    assert {k: int(v[0]) for k, v in Cc.stats().items()} == {k: int(v[1]) for k, v in A.stats().items()}
    assert int(Cc.pending[0]) == int(A.pending[1])


# ---- one real model --------------------------------------------------------------------------------------------------------------------
def test_the_student_scores_the_offline_resampling_of_the_played_out_stream():
    from afx import engine, synth
    from afx.jitter import JitterScorer
    from afx.streaming import KVCachedScorer
    rate, S = 8000, 2
    sd = synth.model_state_dict("ConformerModel", n_layers=1, n_encoders=1)
    eng = engine.Engine("conformer", n_layers=1, dtype="fp16", conf_blocks=1)
    eng.load_state_dict(sd)
    js = JitterScorer(KVCachedScorer(eng, sd, S, window=64000, hop=H), rate, "mulaw", 3 * (rate // 50), conceal="pitch_sync")
    inner = KVCachedScorer(eng, sd, S, window=64000, hop=H)
    rng = random.Random(3)
    sch = [Schedule(rate, "mulaw", 900 + s, jump=js.J + 40, f0=(125, None)[s]) for s in range(S)]
    refs = [Ref(rate, js.depth) for sc in sch]
    scores = [[] for _ in range(S)]
    while not all(sc.done() for sc in sch):
        ticks = {s: sch[s].tick() for s in range(S) if not sch[s].done() and rng.random() < 0.8}
        if not ticks:
            continue
        rows, named = _rows(ticks, rng)
        for s, ts, t, raw, x, e in rows:
            refs[s].packet(t, x)
        res = js.feed([r[3] for r in rows], [r[0] for r in rows], [r[1] for r in rows])
        for r, part in zip(rows, res.split()):
            scores[r[0]].append(part)
        for s in named:
            refs[s].after_feed()
            assert sum(p.numel() for p in scores[s]) == -(-refs[s].next * js.L // js.M) // H  # in the call that releases the hop
    res = js.flush()
    for s, part in zip(range(S), res.split()):
        scores[s].append(part)
    for s in range(S):
        refs[s].release(refs[s].hi)
        whole = _offline(refs[s].E, rate)
        want = torch.cat([inner.push(whole[j * H:(j + 1) * H][None].contiguous(), [s]) for j in range(whole.numel() // H)])
        got = torch.cat(scores[s])
        assert got.numel() == want.numel() >= 5 and torch.equal(bits(got), bits(want)), s
        assert refs[s].stats["concealed"] > 0 and int(js.stats()["concealed"][s]) == refs[s].stats["concealed"]
