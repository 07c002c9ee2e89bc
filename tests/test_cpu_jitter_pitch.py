"""Pitch-period loss concealment, the host side (afx/jitter.py conceal="pitch_sync"): the numpy statement of the function itself
(``pitch_reference``, ``quantize``, ``gain_table``) on the signals it was prototyped on, the geometry it adds to a scorer, the
plans of a host-only scorer (where the estimate goes, and that a "repeat" scorer plans what it planned), the played-out stream
of those plans run on a numpy ring against the per-sample simulation, the refusals of the four entry points and the session
state.  No GPU: the kernels restated in numpy from include/afx.h and the simulation are oracle/jitter.py's ``NumpyDevice`` and
``RefSlot``."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import packet_helpers
from oracle.jitter import NumpyDevice, RefSlot, voiced
from packet_helpers import bits as _bits, go as _go

H = 4000
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F0S = (70, 97, 125, 180, 200, 260, 390)
RATES = (8000, 16000, 48000)


@pytest.fixture(scope="module", autouse=True)
def built():
    return packet_helpers.built()


def _host(S=3, rate=8000, encoding="pcm_f32le", depth=160, **kw):
    from afx.jitter import JitterScorer
    from afx.streaming import SlidingWindowScorer
    return JitterScorer(SlidingWindowScorer(None, S, window=16000, hop=H, device="cpu"), rate, encoding, depth, **kw)


# ---- the reference itself ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", RATES)
def test_the_chosen_lag_is_a_pitch_period_and_continues_the_signal_better_than_a_fixed_10_ms(rate):
    from afx.jitter import gain_table, pitch_lags, pitch_reference
    Pmin, Pmax, Wc = pitch_lags(rate)
    Lh, P0, ten = Pmax + Wc, rate // 100, rate // 100
    fade = (1.0 - np.arange(3 * P0, dtype=np.float64) / (3 * P0)).astype(np.float32)  # "repeat": F = 3 P
    gain = gain_table(rate // 100, rate // 20)
    d = np.arange(ten)
    for f0 in F0S:
        x = voiced(rate, f0, Lh + ten, 1000 * f0 + rate)
        hist, true = x[:Lh], x[Lh:]
        p = pitch_reference(hist, rate)
        T = rate / f0
        assert Pmin <= p <= Pmax and abs(p - round(p / T) * T) <= 1, (rate, f0, p)
        new = gain[d] * hist[Lh - p + d % p]
        old = fade[d] * hist[Lh - P0 + d % P0]
        e_new, e_old = np.abs(new - true).max(), np.abs(old - true).max()
        print(f"rate {rate} f0 {f0}: p* {p}, worst error pitch_sync {e_new:.4f}, repeat {e_old:.4f}")
        if f0 != 200:  # (at 200 Hz 10 ms is a whole number of periods)
            assert e_new < e_old, (rate, f0, e_new, e_old)


def test_silence_gives_the_fallback_and_an_exact_tie_the_smallest_lag():
    from afx.jitter import pitch_lags, pitch_reference
    for rate in (8000, 11025, 48000):
        Pmin, Pmax, Wc = pitch_lags(rate)
        assert pitch_reference(np.zeros(Pmax + Wc, np.float32), rate) == rate // 100
        assert pitch_reference(np.zeros(Pmax + Wc, np.float32), rate, period=Pmin + 1) == Pmin + 1
        assert pitch_reference(np.zeros(0, np.float32), rate) == rate // 100  # (nothing before the origin: zeros)
    g = np.random.default_rng(4)
    x = np.tile(g.integers(-9000, 9000, 40), 8)[:280].astype(np.float32) / np.float32(32768)  # exactly periodic integers: 40
    assert pitch_reference(x, 8000) == 40  # the scores of 40, 80 and 120 tie exactly: the smallest lag
    assert pitch_reference(-x, 8000) == 40 and pitch_reference(np.concatenate([np.zeros(99, np.float32), x]), 8000) == 40


def test_the_quantiser_and_the_gain_table():
    from afx.jitter import gain_table, quantize
    x = np.array([np.nan, np.inf, -np.inf, 3.0, -2.5, 1.0, -1.0, 0.5 / 32768, 1.5 / 32768, 2.5 / 32768, -0.5 / 32768, 0.25, 1e-9],
                 dtype=np.float32)
    assert quantize(x).tolist() == [0, 32767, -32768, 32767, -32768, 32767, -32768, 0, 2, 2, 0, 8192, 0]  # ties to even
    assert quantize(x).dtype == np.int64 and quantize(np.zeros((2, 3), np.float32)).shape == (2, 3)
    big = np.float32(3.0e38)  # (x * 32768 overflows fp32 to +inf: still the clamp)
    assert quantize([big, -big]).tolist() == [32767, -32768]
    g = gain_table(3, 4)
    assert g.dtype == np.float32 and g.tolist() == [1, 1, 1, 1, 0.75, 0.5, 0.25]
    assert gain_table(0, 0).shape == (0,) and gain_table(2, 0).tolist() == [1, 1]
    assert gain_table(80, 400)[81] == np.float32(1.0 - 1 / 400)


# ---- geometry ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,lags,corr,hold,fade,lookback", [(8000, (20, 120), 160, 80, 400, 600), (11025, (27, 165), 220, 110, 551, 826),
                                                                (48000, (120, 720), 960, 480, 2400, 3600)])
def test_geometry_of_a_pitch_sync_scorer(rate, lags, corr, hold, fade, lookback):
    from afx.jitter import CONCEAL
    assert CONCEAL == ("zero", "repeat", "pitch_sync")
    depth = 3 * (rate // 50)
    js = _host(rate=rate, depth=depth, conceal="pitch_sync")
    assert (js.lags, js.corr, js.hold, js.fade_len, js.period) == (lags, corr, hold, fade, rate // 100)
    assert js.rs.T - 1 < lookback and js.lookback == lags[1] + max(corr, hold + fade) == lookback
    W = depth + -(-H * js.M // js.L) + 1
    assert (js.W, js.J) == (W, lookback + W) and js.fade.shape == (hold + fade,) and js.jperiod.tolist() == [0, 0, 0]
    short = _host(rate=rate, depth=depth, conceal="pitch_sync", hold=0, fade=7, period=lags[0])  # the search history governs
    assert short.lookback == max(short.rs.T - 1, lags[1] + corr) and (short.hold, short.fade_len, short.period) == (0, 7, lags[0])
    old = _host(rate=rate, depth=depth)  # "repeat" is sized as it was, and has no part of the new function
    assert old.lookback == max(old.rs.T - 1, 4 * (rate // 100)) and (old.hold, old.lags, old.corr) == (0, (0, 0), 0)
    assert not hasattr(old, "jperiod")


def test_constructor_refusals():
    from afx.jitter import MixedJitterScorer
    from afx.streaming import SlidingWindowScorer
    for kw in (dict(hold=-1), dict(hold=1.5), dict(hold=True), dict(period=19), dict(period=121), dict(fade=-1)):
        with pytest.raises(ValueError):
            _host(conceal="pitch_sync", **kw)
    for kw in (dict(conceal="repeat", hold=80), dict(conceal="zero", hold=0), dict(conceal="pitch"), dict(conceal="pitch", hold=80)):
        with pytest.raises(ValueError):
            _host(**kw)
    assert _host(conceal="repeat", period=1).period == 1 and _host(conceal="repeat", period=500).period == 500  # as before
    assert _host(conceal="pitch_sync", period=20).period == 20 and _host(conceal="pitch_sync", period=120, hold=0).hold == 0
    sc = SlidingWindowScorer(None, 2, window=16000, hop=H, device="cpu")
    fm = [(8000, "mulaw"), (48000, "pcm_f32le")]
    for kw in (dict(conceal="repeat", hold_ms=10), dict(conceal="pitch_sync", hold_ms=-1), dict(conceal="pitch_sync", period_ms=2),
               dict(conceal="pitch_sync", period_ms=16), dict(conceal="pitch")):
        with pytest.raises(ValueError):
            MixedJitterScorer(sc, fm, 60, **kw)
    ms = MixedJitterScorer(sc, fm, 60, conceal="pitch_sync", hold_ms=5, fade_ms=40, period_ms=5)
    assert (ms._rHd.tolist(), ms._rF.tolist(), ms._rP.tolist()) == ([40, 240], [320, 1920], [40, 240])
    ms = MixedJitterScorer(sc, fm, 60, conceal="pitch_sync")
    assert ms._rlookback.tolist() == [600, 3600] and ms._rJ.tolist() == [_host(rate=r, depth=60 * r // 1000, conceal="pitch_sync").J for r, _ in fm]


# ---- plans -------------------------------------------------------------------------------------------------------------------------
def _kinds(plan):
    return [op[0] for op in plan.ops if op[0] != "pop"]


def _feed(js, dev, x, k, n, slot=0):
    """Packet k (n samples of x) of ``slot`` -> the plan, run and committed."""
    plan, pay = js._plan_feed([x[k * n:(k + 1) * n].tobytes()], [slot], [k * n])
    _go(js, dev, plan, pay)
    return plan


def test_a_gap_released_over_three_calls_has_one_pitch_row_at_the_first():
    n, x = 160, voiced(8000, 125, 40 * 160, 5)
    js = _host(S=2, depth=3 * n, conceal="pitch_sync")
    dev, ref = NumpyDevice(js), RefSlot(3 * n, "pitch_sync", rate=8000)
    plans = {}
    for k in [q for q in range(20) if q not in (6, 7, 8, 9)]:  # 80 ms lost: released by the feeds of packets 10, 11 and 12
        plans[k] = _feed(js, dev, x, k, n, slot=1)
        ref.packet(k * n, x[k * n:(k + 1) * n])
        ref.release(max(ref.next, ref.hi - 3 * n))
    assert _kinds(plans[5]) == ["place", "release"] and _kinds(plans[13]) == ["place", "release"]
    assert _kinds(plans[10]) == ["place", "pitch", "conceal", "release"]
    assert _kinds(plans[11]) == ["place", "conceal", "release"] and _kinds(plans[12]) == ["place", "conceal", "release"]
    pitch, conceal = plans[10].ops[1], plans[10].ops[2]
    assert pitch[1].dtype == np.int32 and pitch[1].tolist() == [[1, 6 * n % js.J]] and pitch[2] == 120 + 160
    assert conceal[1].tolist() == [[1, 6 * n % js.J, 0, 2 * n]] and plans[11].ops[1][1].tolist() == [[1, 6 * n % js.J, 2 * n, 3 * n]]
    assert plans[12].ops[1][1].tolist() == [[1, 6 * n % js.J, 3 * n, 4 * n]]  # (3 n = G: the last row is all zeros, not yet past it)
    assert ref.periods == [64] and dev.period.tolist() == [0, 64]  # 8000 / 125
    assert np.array_equal(_bits(dev.out[1]), _bits(ref.E)) and len(ref.E) == 17 * n
    assert np.count_nonzero(ref.E[6 * n:9 * n]) > 2.9 * n and not np.any(ref.E[9 * n:10 * n])


def test_two_gaps_of_one_slot_in_one_release_are_estimated_in_rank_order():
    n, x = 160, voiced(8000, 97, 40 * 160, 6)
    js = _host(S=1, depth=0, conceal="pitch_sync")
    dev, ref = NumpyDevice(js), RefSlot(0, "pitch_sync", rate=8000)
    for k in range(4):
        _feed(js, dev, x, k, n)
    # packets 4 and 6 lost, 5 and 7 in one feed: the second gap's history holds the first gap's concealed samples
    plan, pay = js._plan_feed([x[7 * n:8 * n].tobytes(), x[5 * n:6 * n].tobytes()], [0, 0], [7 * n, 5 * n])
    _go(js, dev, plan, pay)
    assert _kinds(plan) == ["place", "pitch", "conceal", "pitch", "conceal", "release"]
    assert [op[1].tolist() for op in plan.ops[1:5]] == [[[0, 4 * n]], [[0, 4 * n, 0, n]], [[0, 6 * n]], [[0, 6 * n, 0, n]]]
    for k in (0, 1, 2, 3, 5, 7):
        ref.packet(k * n, x[k * n:(k + 1) * n])
    ref.release(8 * n)
    assert np.array_equal(_bits(dev.out[0]), _bits(ref.E)) and len(ref.periods) == 2 and int(dev.period[0]) == ref.periods[1]


def test_a_row_past_hold_and_fade_is_rebased_and_has_no_pitch():
    n, x = 160, voiced(8000, 180, 40 * 160, 7)
    js = _host(S=1, depth=0, conceal="pitch_sync", hold=40, fade=100)
    dev, ref = NumpyDevice(js), RefSlot(0, "pitch_sync", rate=8000, hold=40, fade=100)
    for k in range(3):
        _feed(js, dev, x, k, n)
    adv = js._plan([0], mode="advance", upto=3 * n + 100)  # the gap opens: d in [0, 100)
    _go(js, dev, adv)
    assert _kinds(adv) == ["pitch", "conceal", "release"] and adv.ops[1][1].tolist() == [[0, 3 * n, 0, 100]]
    adv = js._plan([0], mode="advance", upto=3 * n + 200)  # d in [100, 200): across G = 140
    _go(js, dev, adv)
    assert _kinds(adv) == ["conceal", "release"] and adv.ops[0][1].tolist() == [[0, 3 * n, 100, 200]]
    adv = js._plan([0], mode="advance", upto=3 * n + 500)  # d in [200, 500): all zeros, counted from a + d_lo - G
    _go(js, dev, adv)
    assert _kinds(adv) == ["conceal", "release"] and adv.ops[0][1].tolist() == [[0, 3 * n + 200 - 140, 140, 440]]
    for k in range(3):
        ref.packet(k * n, x[k * n:(k + 1) * n])
    ref.release(3 * n + 500)
    assert np.array_equal(_bits(dev.out[0]), _bits(ref.E)) and not np.any(ref.E[3 * n + 140:]) and np.count_nonzero(ref.E[3 * n:3 * n + 140]) > 130


def test_a_repeat_scorer_plans_what_it_planned():
    """The "repeat" plan of this traffic, row by row as the planner before this mode made it (written out here), and no
    "pitch" op; the "pitch_sync" plan of the same traffic is that plan with the estimate before each gap's first conceal."""
    from afx.ingest import plan as ingest_plan
    n, x = 160, voiced(8000, 125, 12 * 160, 8)
    old, new = _host(S=2, depth=n), _host(S=2, depth=n, conceal="pitch_sync")
    assert (old.period, old.fade_len, old.lookback) == (80, 240, 320)
    made = 0
    for k in (0, 1, 3, 4, 7):  # packet 2 lost; 5 and 6 lost: a gap of 320 > P + F released in one call
        po, pay = old._plan_feed([x[k * n:(k + 1) * n].tobytes()], [1], [k * n])
        pn, _ = new._plan_feed([x[k * n:(k + 1) * n].tobytes()], [1], [k * n])
        J = old.J
        want = [("place", [[1, 0, n, k * n % J]], n)]
        lo, hi = max(0, (k - 1) * n - (n if k in (3, 7) else 0) - (n if k == 7 else 0)), k * n  # what this feed releases
        if k == 3:
            want.append(("conceal", [[1, 2 * n % J, 0, n]], n))
        if k == 7:
            want.append(("conceal", [[1, 5 * n % J, 0, 2 * n]], 2 * n))
        if hi > lo:
            n_out, p0, d0 = ingest_plan(lo, hi - lo, old.L, old.M)
            want.append(("release", [[1, lo % J, hi - lo, n_out, p0, d0, made % old.ring_len, 0]], n_out))
            made += n_out
        got = [(op[0], op[1].tolist(), op[2]) for op in po.ops if op[0] != "pop"]
        assert got == want, (k, got, want)
        assert all(op[1].dtype == np.int32 for op in po.ops if op[0] != "pop")
        kinds = _kinds(pn)
        assert [q for q in kinds if q != "pitch"] == _kinds(po) and kinds.count("pitch") == (1 if k in (3, 7) else 0)
        if "pitch" in kinds:
            assert kinds[kinds.index("pitch") + 1] == "conceal"
        assert [op[2] for op in po.ops if op[0] == "pop"] == [op[2] for op in pn.ops if op[0] == "pop"]
        old._commit(po.book)
        new._commit(pn.book)
    assert old.stats()["concealed"].tolist() == new.stats()["concealed"].tolist() == [0, 3 * n]


def test_a_lossy_stream_of_a_host_scorer_equals_the_per_sample_simulation():
    import random
    from afx.jitter import MixedJitterScorer
    from afx.streaming import SlidingWindowScorer
    rng = random.Random(11)
    ms = MixedJitterScorer(SlidingWindowScorer(None, 2, window=16000, hop=H, device="cpu"), [(8000, "pcm_f32le"), (11025, "pcm_f32le")],
                           40, conceal="pitch_sync")
    ms.reset([0, 1], [11025, 8000])
    one = _host(S=1, rate=11025, depth=40 * 11025 // 1000, conceal="pitch_sync")
    devs, rates = (NumpyDevice(ms), NumpyDevice(one)), (11025, 8000)
    refs = [RefSlot(40 * r // 1000, "pitch_sync", rate=r) for r in rates]
    xs = [voiced(r, f, 50 * (r // 50), 9) for r, f in zip(rates, (180, 97))]
    lost = [{k for k in range(3, 50) if rng.random() < 0.2} | {20, 21, 22, 23, 24}, {k for k in range(3, 50) if rng.random() < 0.2}]
    for k0 in range(0, 50, 2):
        # (packet 0 first: it is the session's origin; later pairs in either order, inside the depth)
        rows = [(s, k) for s in (0, 1) for k in (rng.sample([k0, k0 + 1], 2) if k0 else [0, 1]) if k not in lost[s]]
        if not rows:
            continue
        pk = [xs[s][k * (rates[s] // 50):(k + 1) * (rates[s] // 50)] for s, k in rows]
        plan, pay = ms._plan_feed([p.tobytes() for p in pk], [s for s, _ in rows], [k * (rates[s] // 50) for s, k in rows])
        _go(ms, devs[0], plan, pay)
        mine = [i for i, (s, _) in enumerate(rows) if s == 0]
        if mine:  # the one-rate scorer of slot 0's rate, fed its packets in the same calls
            plan, pay = one._plan_feed([pk[i].tobytes() for i in mine], [0] * len(mine), [rows[i][1] * (11025 // 50) for i in mine])
            _go(one, devs[1], plan, pay)
        for (s, k), p in zip(rows, pk):
            refs[s].packet(k * (rates[s] // 50), p)
        for s in {s for s, _ in rows}:
            refs[s].release(max(refs[s].next, refs[s].hi - refs[s].depth))
    for s in (0, 1):
        assert np.array_equal(_bits(devs[0].out[s]), _bits(refs[s].E)) and len(refs[s].periods) >= 4
        assert any(p != rates[s] // 100 for p in refs[s].periods)
    assert np.array_equal(_bits(devs[1].out[0]), _bits(refs[0].E)) and int(devs[1].period[0]) == int(devs[0].period[0])
    assert devs[0].launches.count("pitch") >= 4 and "pitch" in devs[1].launches


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------
def test_the_four_entry_points_are_declared_exported_and_refuse_by_name(built):
    from afx._lib import JitterLags, JitterRate
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "afx.h")).read(), flags=re.S)
    so = ctypes.CDLL(built.LIB_PATH)
    for name, nargs in (("afx_k_jitter_pitch", 11), ("afx_k_jitter_pitch_rates", 10), ("afx_k_jitter_conceal_period", 14),
                        ("afx_k_jitter_conceal_period_rates", 11)):
        assert re.search(r"\b%s\s*\(" % name, src) and hasattr(so, name) and len(built.SIGNATURES[name][1]) == nargs
    assert re.search(r"typedef struct afx_jitter_rate \{[^}]*const float\* taps;[^}]*const float\* fade;[^}]*int L, M, T, J, P, F;\s*\}", src)
    assert ctypes.sizeof(JitterRate) == 40 and ctypes.sizeof(JitterLags) == 20  # (afx_jitter_rate's layout is unchanged)
    l = built.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def table(n=1, **kw):
        rates, lags = (JitterRate * n)(), (JitterLags * n)()
        for r, g in zip(rates, lags):
            v = dict(dict(taps=None, fade=p, L=1, M=1, T=1, J=64, P=8, F=6, Pmin=4, Pmax=16, Wc=20, P0=8, Hd=2), **kw)
            for k in ("taps", "fade", "L", "M", "T", "J", "P", "F"):
                setattr(r, k, v[k])
            for k in ("Pmin", "Pmax", "Wc", "P0", "Hd"):
                setattr(g, k, v[k])
        return ctypes.cast(rates, ctypes.c_void_p), ctypes.cast(lags, ctypes.c_void_p)

    def pitch(jring=p, S=1, J=64, hdr=p, rows=1, Pmin=4, Pmax=16, Wc=20, P0=8, period=p):
        return l.afx_k_jitter_pitch(jring, S, J, hdr, rows, Pmin, Pmax, Wc, P0, period, None)

    def pitch_rates(jring=p, S=1, Js=64, hdr=p, rows=1, t=None, n=1, period=p, **kw):
        rates, lags = table(n if 1 <= n <= 16 else 1, **kw) if t is None else t
        return l.afx_k_jitter_pitch_rates(jring, S, Js, hdr, rows, rates, lags, n, period, None)

    def synth(jring=p, S=1, J=64, hdr=p, rows=1, max_n=8, gain=p, period=p, Pmin=4, Pmax=16, P0=8, Hd=2, F=6):
        return l.afx_k_jitter_conceal_period(jring, S, J, hdr, rows, max_n, gain, period, Pmin, Pmax, P0, Hd, F, None)

    def synth_rates(jring=p, S=1, Js=64, hdr=p, rows=1, max_n=8, t=None, n=1, period=p, **kw):
        rates, lags = table(n if 1 <= n <= 16 else 1, **kw) if t is None else t
        return l.afx_k_jitter_conceal_period_rates(jring, S, Js, hdr, rows, max_n, rates, lags, n, period, None)

    cases = [
        (pitch, dict(jring=None), b"null"), (pitch, dict(hdr=None), b"null"), (pitch, dict(period=None), b"null"),
        (pitch, dict(rows=0), b"rows"), (pitch, dict(rows=65536), b"rows"), (pitch, dict(Pmin=0), b"Pmin"),
        (pitch, dict(Pmax=3), b"Pmax"), (pitch, dict(Wc=0), b"Wc"), (pitch, dict(P0=3), b"P0"), (pitch, dict(P0=17), b"P0"),
        (pitch, dict(J=35), b"history"), (pitch, dict(Pmax=30000, Wc=30000, J=1 << 20), b"LDS"),
        (synth, dict(jring=None), b"null"), (synth, dict(hdr=None), b"null"), (synth, dict(period=None), b"null"),
        (synth, dict(gain=None), b"gain"), (synth, dict(rows=0), b"rows"), (synth, dict(rows=65536), b"rows"),
        (synth, dict(Pmin=0), b"Pmin"), (synth, dict(Pmax=3), b"Pmax"), (synth, dict(P0=3), b"P0"), (synth, dict(P0=17), b"P0"),
        (synth, dict(Hd=-1), b"hold"), (synth, dict(F=-1), b"hold"), (synth, dict(max_n=49), b"fit"), (synth, dict(max_n=-1), b"fit"),
        (pitch_rates, dict(n=0), b"1 to 16 rates"), (pitch_rates, dict(n=17), b"1 to 16 rates"),
        (pitch_rates, dict(t=(None, table()[1])), b"null rate table"), (pitch_rates, dict(t=(table()[0], None)), b"null rate table"),
        (pitch_rates, dict(jring=None), b"null"), (pitch_rates, dict(period=None), b"null"), (pitch_rates, dict(rows=65536), b"rows"),
        (pitch_rates, dict(Pmin=0), b"Pmin"), (pitch_rates, dict(Pmax=3), b"Pmax"), (pitch_rates, dict(Wc=0), b"Wc"),
        (pitch_rates, dict(P0=17), b"P0"), (pitch_rates, dict(J=35), b"history"), (pitch_rates, dict(n=2, J=35), b"history"),
        (pitch_rates, dict(J=65), b"1 <= J <= Js"), (pitch_rates, dict(J=0), b"1 <= J <= Js"), (pitch_rates, dict(L=0), b"bad filter shape"),
        (pitch_rates, dict(L=2), b"identity"), (pitch_rates, dict(taps=p, T=66), b"filter history"),
        (synth_rates, dict(n=0), b"1 to 16 rates"), (synth_rates, dict(t=(table()[0], None)), b"null rate table"),
        (synth_rates, dict(hdr=None), b"null"), (synth_rates, dict(rows=0), b"rows"), (synth_rates, dict(fade=None), b"gain"),
        (synth_rates, dict(Pmin=0), b"Pmin"), (synth_rates, dict(Pmax=3), b"Pmax"), (synth_rates, dict(Wc=0), b"Wc"),
        (synth_rates, dict(P0=3), b"P0"), (synth_rates, dict(Hd=-1), b"hold"), (synth_rates, dict(max_n=49), b"fit"),
        (synth_rates, dict(Js=63), b"1 <= J <= Js"), (synth_rates, dict(M=0), b"bad filter shape"),
    ]
    names = {pitch: b"jitter_pitch:", pitch_rates: b"jitter_pitch_rates:", synth: b"jitter_conceal_period:",
             synth_rates: b"jitter_conceal_period_rates:"}
    for fn, kw, word in cases:
        assert fn(**kw) != 0, (fn.__name__, kw)
        msg = l.afx_last_error()
        assert word in msg and msg.startswith(names[fn]), (fn.__name__, kw, msg)
    # the existing entry points still refuse mode 2, by the word the existing tests look for
    assert l.afx_k_jitter_conceal(p, 1, 16, p, 1, 1, p, 8, 4, 2, None) != 0 and b"mode" in l.afx_last_error()


# ---- sessions ------------------------------------------------------------------------------------------------------------------------
def _open_gap(js, dev, slot, n=160):
    """Packets 0..3, then an advance 100 samples into the gap after them: an open gap of age 100 < hold + fade."""
    x = voiced(8000, 125, 4 * n, 12)
    for k in range(4):
        _feed(js, dev, x, k, n, slot)
    _go(js, dev, js._plan([slot], mode="advance", upto=4 * n + 100))


def test_the_period_of_an_open_gap_moves_with_its_session():
    from afx.jitter import MixedJitterScorer
    from afx.streaming import SlidingWindowScorer
    js = _host(S=3, depth=160, conceal="pitch_sync")
    dev = NumpyDevice(js)
    _open_gap(js, dev, 2)
    assert js.jperiod.tolist() == [0, 0, 64]
    js.jperiod[0] = 99  # (a slot without an open gap: whatever is stored is masked)
    st = js.export_slots([2, 0])
    assert st.tensors["jitter_pitch"].dtype == torch.int64 and st.tensors["jitter_pitch"].tolist() == [64, 0]
    assert st.meta["jitter_conceal"] == "pitch_sync" and st.meta["jitter_hold"] == 80 and st.meta["jitter_lags"] == (20, 120, 160)
    assert (st.meta["jitter_period"], st.meta["jitter_fade"]) == (80, 400) and st.tensors["jitter_ring"].shape == (2, 600 + 160)
    other = _host(S=2, depth=160, conceal="pitch_sync")
    other.import_slots([1, 0], st)
    assert other.jperiod.tolist() == [0, 64] and other.export_slots([1]).tensors["jitter_pitch"].tolist() == [64]
    # ... and the gap goes on in the new scorer with that period: the same samples as in the old one
    a, b = NumpyDevice(js), NumpyDevice(other)
    a.N[2] = b.N[1] = 4 * 160 + 100  # (the playout counter of the session both devices take up)
    _go(js, a, js._plan([2], mode="advance", upto=4 * 160 + 300))
    _go(other, b, other._plan([1], mode="advance", upto=4 * 160 + 300))
    assert len(a.out[2]) == 200 and np.array_equal(_bits(a.out[2]), _bits(b.out[1])) and np.count_nonzero(a.out[2]) > 190
    # a gap that still sounds with a period outside the lags, and a period no slot can hold, are refused; nothing changes
    for bad in (19, 0, 121, -3):
        st.tensors["jitter_pitch"] = torch.tensor([bad, 0])
        with pytest.raises(ValueError, match="jitter_pitch"):
            _host(S=2, depth=160, conceal="pitch_sync").import_slots([0, 1], st)
    st.tensors["jitter_pitch"] = torch.tensor([64, 0], dtype=torch.int32)
    with pytest.raises(ValueError, match="jitter_pitch"):
        _host(S=2, depth=160, conceal="pitch_sync").import_slots([0, 1], st)
    st.tensors["jitter_pitch"] = torch.tensor([64, 0])
    for kw in (dict(hold=81), dict(fade=401), dict(period=81), dict(depth=161)):
        with pytest.raises(ValueError):
            _host(S=2, **dict(dict(depth=160, conceal="pitch_sync"), **kw)).import_slots([0, 1], st)
    # the modes refuse each other, in both directions; a "repeat" state has none of the new keys
    for mode in ("repeat", "zero"):
        with pytest.raises(ValueError):
            _host(S=2, depth=160, conceal=mode).import_slots([0, 1], st)
        old = _host(S=2, depth=160, conceal=mode).export_slots([0, 1])
        assert "jitter_pitch" not in old.tensors and not {"jitter_hold", "jitter_lags"} & set(old.meta)
        with pytest.raises(ValueError):
            _host(S=2, depth=160, conceal="pitch_sync").import_slots([0, 1], old)
    # a mixed scorer takes the plain state where rate and parameters match, and gives it back per session
    sc = SlidingWindowScorer(None, 2, window=16000, hop=H, device="cpu")
    ms = MixedJitterScorer(sc, [(48000, "pcm_f32le"), (8000, "pcm_f32le")], 20, conceal="pitch_sync")
    ms.import_slots([1, 0], st)
    assert ms.rates.tolist() == [8000, 8000] and ms.jperiod.tolist() == [0, 64]
    back = ms.export_slots([1])
    assert back.tensors["jitter_pitch"].tolist() == [64] and back.tensors["jitter_params"].tolist() == [[160, 80, 400, 80]]
    ms2 = MixedJitterScorer(sc, [(8000, "pcm_f32le")], 20, conceal="pitch_sync")
    ms2.import_slots([0], back)
    assert ms2.jperiod.tolist() == [64, 0]
    with pytest.raises(ValueError):
        MixedJitterScorer(sc, [(8000, "pcm_f32le")], 20, conceal="pitch_sync", hold_ms=5).import_slots([0], st)
    with pytest.raises(ValueError):
        MixedJitterScorer(sc, [(8000, "pcm_f32le")], 20, conceal="repeat").import_slots([0], back)
    js.reset([2])
    assert js.jperiod.tolist() == [99, 0, 0]
