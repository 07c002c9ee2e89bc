"""Comfort noise on the GPU (afx/jitter.py ``ComfortNoise``; afx_k_jitter_noise / _noise_rates).  The kernel alone, bit for
bit against ``ComfortNoise.samples`` on a ring prefilled with a sentinel, every row-skip case included; the played-out stream
of a DTX call (talk spurts, CN marks, lost CNs and lost last packets, late marks, ``advance`` through a silence) against the
offline resampling of the per-sample numpy stream; the scores against a fresh inner scorer pushed that stream; a session moved
in mid-silence; and ``feed_rtp`` with CN datagrams and an ignored telephone-event type.  The per-sample reference and the
traffic are oracle/jitter.py's ``RefSlot`` and ``dtx_events``."""
import ctypes
import io
import random

import numpy as np
import pytest
import torch

from oracle.jitter import RefSlot, TABLES, dtx_events, rtp as _rtp
from packet_helpers import bits as _bits, offline as _offline, tap as _tap

pytestmark = pytest.mark.gpu

H = 4000
SENTINEL = 7.5


def _encoded(events, encoding, seed):
    """The traffic of ``dtx_events`` with its packets as ``encoding``: ("pkt", t, bytes, decoded fp32) / ("cn", t, level)."""
    g, out = np.random.default_rng(seed), []
    for kind, t, v in events:
        if kind == "cn":
            out.append((kind, t, v))
        elif encoding == "mulaw":
            c = g.integers(0, 256, len(v)).astype(np.uint8)
            out.append((kind, t, c.tobytes(), TABLES["mulaw"][c]))
        else:
            q = (g.integers(-32768, 32768, len(v)) // 8).astype("<i2")
            out.append((kind, t, q.tobytes(), q.astype(np.float32) / np.float32(32768)))
    return out


# ---- the kernel alone -------------------------------------------------------------------------------------------------------------
def _launch(fn, ring, rows, max_n, seed, amp, *table):
    from afx._lib import call_on, check, ptr
    hdr = torch.tensor(rows, dtype=torch.int64).to(torch.int32).cuda()  # (lo32 keeps its bits)
    S, J = ring.shape
    check(call_on(ring, fn, ptr(ring), S, J, ptr(hdr), len(rows), max_n, *table, seed, ptr(amp)))
    torch.cuda.synchronize()
    return ring.cpu().numpy()


def _lo_hi(i0):
    lo = i0 & 0xFFFFFFFF
    return [lo - (1 << 32) if lo >= 1 << 31 else lo, i0 >> 32]


def _expect(ring, cn, J, rows):
    for slot, c, n, i0, level in rows:
        ring[slot, (c + np.arange(n)) % J] = cn.samples(i0, n, level)
    return ring


def test_noise_kernel_alone_is_bit_for_bit_the_numpy_statement():
    from afx._lib import JitterRate, lib
    from afx.jitter import ComfortNoise
    S, J, seed = 3, 1000, 0x9E3779B1
    cn = ComfortNoise(seed)
    amp = torch.from_numpy(cn.amp).cuda()
    l = lib()
    fresh = lambda: torch.full((S, J), SENTINEL, dtype=torch.float32, device="cuda")
    # n = 0, 1, 257 and J; a wrap (c + n > J); i0 = 2^32 - 100 with n = 257 (crosses into the high half); levels 0, 60, 127;
    # two (here three) rows of one slot
    good = [(0, 10, 1, 5, 0), (0, 100, 257, (1 << 32) - 100, 60), (0, 700, 0, 9, 60), (1, 900, 257, 123456789012, 127), (2, 333, J, 77, 60)]
    rows = [[s, c, n] + _lo_hi(i0) + [lv] for s, c, n, i0, lv in good]
    got = _launch(l.afx_k_jitter_noise, fresh(), rows, J, seed, amp)
    want = _expect(np.full((S, J), SENTINEL, dtype=np.float32), cn, J, good)
    assert np.array_equal(_bits(got), _bits(want))
    assert (got[0] == SENTINEL).sum() == J - 258 and (got[1] == SENTINEL).sum() == J - 257 and not (got[2] == SENTINEL).any()
    assert not np.array_equal(got[0, 100:357], cn.samples(1 << 32, 257, 60)[:257]) and got[0, 200] == cn.samples(1 << 32, 1, 60)[0]
    # every row-skip case leaves the sentinel; the one good row of the launch is written
    skips = [[-1, 0, 5, 0, 0, 60], [S, 0, 5, 0, 0, 60], [0, -1, 5, 0, 0, 60], [0, J, 5, 0, 0, 60], [0, 0, -1, 0, 0, 60], [0, 0, J + 1, 0, 0, 60],
             [1, 0, 5, 0, 0, -1], [1, 0, 5, 0, 0, 128], [1, 0, 5, 0, -1, 60], [2, 40, 9, 3, 0, 127]]
    got = _launch(l.afx_k_jitter_noise, fresh(), skips, J, seed, amp)
    want = _expect(np.full((S, J), SENTINEL, dtype=np.float32), cn, J, [(2, 40, 9, 3, 127)])
    assert np.array_equal(_bits(got), _bits(want)) and (got != SENTINEL).sum() == 9
    # the _rates form: two rates of different J in one launch, each wrapping at its own J; a bad rate index is skipped
    table = (JitterRate * 2)()
    for t, Jf in zip(table, (J, 600)):
        t.taps, t.fade, t.L, t.M, t.T, t.J, t.P, t.F = None, None, 1, 1, 1, Jf, 0, 0
    tp = ctypes.cast(table, ctypes.c_void_p)
    rated = [(0, 900, 200, 5000, 60, 0), (1, 500, 200, (1 << 33) + 7, 30, 1), (2, 590, 20, 1, 60, 1)]
    rows = [[s, c, n] + _lo_hi(i0) + [lv, r] for s, c, n, i0, lv, r in rated]
    rows += [[2, 0, 5, 0, 0, 60, -1], [2, 0, 5, 0, 0, 60, 2], [1, 600, 5, 0, 0, 60, 1], [1, 0, 601, 0, 0, 60, 1]]  # (c, n beyond the row's own J)
    got = _launch(l.afx_k_jitter_noise_rates, fresh(), rows, 601, seed, amp, tp, 2)
    want = np.full((S, J), SENTINEL, dtype=np.float32)
    for (s, c, n, i0, lv, r), Jf in zip(rated, (J, 600, 600)):
        want[s, (c + np.arange(n)) % Jf] = cn.samples(i0, n, lv)
    assert np.array_equal(_bits(got), _bits(want)) and (got[1:, 600:] == SENTINEL).all() and (got[1, :100] != SENTINEL).all()


# ---- the played-out stream ------------------------------------------------------------------------------------------------------------
class _Call:
    """A comfort-noise JitterScorer over ``inner`` driven by the DTX traffic of each slot, and the per-sample reference."""

    def __init__(self, inner, S, rate, encoding, mode, seed, cn_seed=77, n_spurts=5, **kw):
        from afx.jitter import ComfortNoise, JitterScorer
        self.rate, self.depth = rate, 3 * (rate // 50)
        self.js = JitterScorer(inner, rate, encoding, self.depth, conceal=mode, comfort_noise=ComfortNoise(cn_seed), **kw)
        self.refs = [RefSlot(self.depth, mode, self.js.period, self.js.fade_len, noise=cn_seed) for _ in range(S)]
        self.ev = [_encoded(dtx_events(rate, seed + 31 * s, n_spurts), encoding, seed + s) for s in range(S)]
        self.origin = [(1 << 32) - 4 * (rate // 50) - 1] + [1000 * s for s in range(1, S)]
        self.at, self.silent = [0] * S, [False] * S
        self.rng = random.Random(seed)

    def done(self):
        return all(a >= len(e) for a, e in zip(self.at, self.ev))

    def step(self, slots=None):
        """One call with the next 1..3 events of some slots -> (result or None, the named slots in order)."""
        rng, rows = self.rng, []
        for s in range(len(self.ev)) if slots is None else slots:
            if self.at[s] < len(self.ev[s]) and (slots is not None or rng.random() < 0.75):
                m = rng.randint(1, 3)
                rows += [(s,) + e for e in self.ev[s][self.at[s]:self.at[s] + m]]
                self.at[s] += m
                self.silent[s] = rows[-1][1] == "cn"
        marks = [r for r in rows if r[1] == "cn"]
        audio = [r for r in rows if r[1] == "pkt"]
        for s, _, t, level in marks:
            self.refs[s].mark(t, level)
        if marks:
            self.js.silence([r[0] for r in marks], [(self.origin[r[0]] + r[2]) % (1 << 32) for r in marks], [r[3] for r in marks])
        if not audio:
            return None, []
        named = []
        for s, _, t, raw, x in audio:
            self.refs[s].packet(t, x)
            named += [s] if s not in named else []
        for s in named:
            self.refs[s].after_feed()
        res = self.js.feed([r[3] for r in audio], [r[0] for r in audio], [(self.origin[r[0]] + r[2]) % (1 << 32) for r in audio])
        return res, named

    def advance(self, s, upto):
        self.refs[s].release(max(self.refs[s].next, upto))
        return self.js.advance([s], upto)

    def flush(self):
        for r in self.refs:
            r.release(r.hi)
        return self.js.flush()

    def stats_equal(self, by_seq=False):
        st = self.js.stats()
        for s, r in enumerate(self.refs):
            got = {k: int(v[s]) for k, v in st.items()}
            assert {k: v for k, v in got.items() if not (by_seq and k == "out_of_order")} == \
                {k: v for k, v in r.stats.items() if not (by_seq and k == "out_of_order")}, (s, got, r.stats)


@pytest.mark.parametrize("mode", ["repeat", "zero"])
@pytest.mark.parametrize("rate,encoding", [(8000, "mulaw"), (16000, "pcm_s16le")])
def test_played_out_dtx_stream_is_the_offline_resampling_of_the_numpy_stream(rate, encoding, mode):
    S = 3
    tap = _tap(S)
    c = _Call(tap, S, rate, encoding, mode, seed=rate // 100 + len(mode), max_pending=3)
    js, pieces = c.js, 0
    while not c.done():
        c.step()
        for s in range(S):  # clock-driven playout through a silence, in several pieces
            if c.silent[s] and c.refs[s].started and c.rng.random() < 0.4:
                for piece in (37, rate // 25, js.J + 50) if pieces % 3 == 0 else (rate // 50,):
                    c.advance(s, c.refs[s].hi + piece - c.depth // 2)
                pieces += 1
    c.flush()
    c.stats_equal()
    for s, r in enumerate(c.refs):
        got = torch.cat(tap.got[s])
        made = -(-r.next * js.L // js.M)
        assert got.numel() == made // H * H >= 2 * H and int(js.pending[s]) == made % H
        assert torch.equal(got, _offline(r.E, rate)[:got.numel()]), s
        assert r.stats["comfort"] > rate // 4 and r.stats["concealed"] > 0 and r.stats["marks"] >= 4
    assert pieces >= 3 and sum(r.stats["marks_late"] for r in c.refs) > 0


# ---- scores ---------------------------------------------------------------------------------------------------------------------------
_ENGINES = {}


def _inner(kind, S):
    from afx import engine, synth
    from afx.streaming import KVCachedScorer, SlidingWindowScorer
    if "e" not in _ENGINES:
        sd = synth.model_state_dict("ConformerModel", n_layers=1, n_encoders=1)
        eng = engine.Engine("conformer", n_layers=1, dtype="fp16", conf_blocks=1)
        eng.load_state_dict(sd)
        _ENGINES["e"] = (eng, sd)
    eng, sd = _ENGINES["e"]
    if kind == "sliding":
        return SlidingWindowScorer(eng, S, window=16000, hop=H, state_dict=sd)
    return KVCachedScorer(eng, sd, S, window=64000, hop=H)


@pytest.mark.parametrize("kind", ["sliding", "kv"])
def test_dtx_scores_equal_the_inner_scorer_on_the_offline_stream(kind):
    S, rate = 3, 8000
    c = _Call(_inner(kind, S), S, rate, "mulaw", "repeat", seed=5 + len(kind), n_spurts=6)
    R = _inner(kind, S)
    checked = [0] * S

    def check(res, named):
        at = 0  # (the scores of a call: the first named slot's in hop order, then the second's, ...)
        assert int(res.counts.sum()) == res.scores.numel() == sum(-(-c.refs[s].next * c.js.L // c.js.M) // H - checked[s] for s in named)
        for s in named:
            want = -(-c.refs[s].next * c.js.L // c.js.M) // H - checked[s]  # every hop whose last sample this call released
            offline = _offline(c.refs[s].E, rate) if want else None
            for j in range(want):
                ref = R.push(offline[checked[s] * H:(checked[s] + 1) * H][None].contiguous(), [s])
                assert torch.equal(res.scores[at:at + 1], ref), (s, checked[s])
                checked[s] += 1
                at += 1

    while not c.done():
        res, named = c.step()
        if res is not None:
            check(res, named)
        s = c.rng.randrange(S)
        if c.silent[s] and c.refs[s].started and c.rng.random() < 0.3:
            check(c.advance(s, c.refs[s].hi + rate // 10), [s])
    check(c.flush(), list(range(S)))
    c.stats_equal()
    assert min(checked) >= 2 and all(r.stats["comfort"] > 0 for r in c.refs)


# ---- a session moved in mid-silence -------------------------------------------------------------------------------------------------------
def test_a_session_moved_on_the_device_in_mid_silence_continues_bit_for_bit():
    from afx.jitter import ComfortNoise, JitterScorer
    from afx.streaming import StreamState
    rate = 8000
    ta, tb = _tap(2), _tap(3)
    c = _Call(ta, 2, rate, "mulaw", "repeat", seed=12, n_spurts=6)
    A = c.js
    B = JitterScorer(tb, rate, "mulaw", c.depth, comfort_noise=ComfortNoise(77), max_pending=5)
    r = c.refs[0]
    while not (r.gap is not None and r.level >= 0 and r.hi > r.next and r.next > H):
        assert not c.done()
        c.step([0, 1])
    st = A.export_slots([0])
    assert int(st.tensors["jitter_cn_open"][0]) == r.level and st.meta["jitter_cn"] == 77
    assert st.tensors["jitter_cn_marks"][0].tolist()[:len(r.marks)] == sorted([t, l] for t, l in r.marks.items())
    buf = io.BytesIO()
    torch.save(st.to("cpu").state_dict(), buf)
    buf.seek(0)
    B.import_slots([2], StreamState.from_state_dict(torch.load(buf, weights_only=True)))
    with pytest.raises(ValueError, match="jitter_cn"):
        JitterScorer(_tap(1), rate, "mulaw", c.depth, comfort_noise=ComfortNoise(78)).import_slots([0], st)
    with pytest.raises(ValueError, match="no ComfortNoise"):
        JitterScorer(_tap(1), rate, "mulaw", c.depth).import_slots([0], st)
    n_a = len(ta.got[0])
    c.js = B  # the rest of slot 0's traffic goes to slot 2 of B: the slot index is no part of the function
    c.refs, c.ev, c.origin, c.at, c.silent = [None, None, r], [[], [], c.ev[0]], [0, 0, c.origin[0]], [0, 0, c.at[0]], [False] * 3
    for i in (0, 1):
        c.refs[i] = RefSlot(c.depth, "repeat", B.period, B.fade_len, noise=77)
    while not c.done():
        c.step([2])
        if c.silent[2] and c.rng.random() < 0.3:
            c.advance(2, r.hi + 100)
    c.flush()
    got = torch.cat(ta.got[0][:n_a] + tb.got[2])
    assert len(tb.got[2]) >= 2 and torch.equal(got, _offline(r.E, rate)[:got.numel()])
    assert {k: int(v[2]) for k, v in B.stats().items()} == r.stats and int(B.samples_in[2]) == r.next


# ---- RTP ------------------------------------------------------------------------------------------------------------------------------
def test_feed_rtp_with_comfort_noise_and_an_ignored_telephone_event_type():
    S, rate = 2, 8000
    ta = _tap(S)
    c = _Call(ta, S, rate, "mulaw", "repeat", seed=21)
    js, seq = c.js, [0] * S
    with pytest.raises(ValueError, match="payload type 101"):
        js.feed_rtp([_rtp(1, 0, pt=101, payload=b"\x01\x00\x00\xa0")], [0])
    while not c.done():
        rows = []
        for s in range(S):
            if c.at[s] < len(c.ev[s]) and c.rng.random() < 0.8:
                for e in c.ev[s][c.at[s]:c.at[s] + 2]:
                    seq[s] += 1
                    ts = (c.origin[s] + e[1]) % (1 << 32)
                    if e[0] == "cn":
                        rows.append((s, _rtp(seq[s], ts, pt=13, payload=bytes([e[2] | 0x80, 9, 9]), ssrc=40 + s), e))
                    else:
                        rows.append((s, _rtp(seq[s], ts, pt=0, payload=e[2], ssrc=40 + s), e))
                        if seq[s] % 7 == 0:  # a DTMF event beside the audio (RFC 4733): parsed, SSRC-checked, dropped
                            rows.append((s, _rtp(seq[s], ts, pt=101, payload=b"\x05\x0a\x00\xa0", ssrc=40 + s), None))
                c.at[s] += 2
        if not rows:
            continue
        for s, _, e in rows:  # the marks of a call are registered before its audio
            if e is not None and e[0] == "cn":
                c.refs[s].mark(e[1], e[2])
        named = []
        for s, _, e in rows:
            if e is not None and e[0] == "pkt":
                c.refs[s].packet(e[1], e[3], by_seq=True)
                named += [s] if s not in named else []
        for s in named:
            c.refs[s].after_feed()
        res = js.feed_rtp([r[1] for r in rows], [r[0] for r in rows], ignore_types=(101,))
        assert res.counts.shape == (len(rows),)
        for (s, _, e), n in zip(rows, res.counts.tolist()):
            assert n == 0 or (e is not None and e[0] == "pkt")  # marks and ignored datagrams count no hops
    c.flush()
    c.stats_equal(by_seq=True)
    for s, r in enumerate(c.refs):
        got = torch.cat(ta.got[s])
        assert got.numel() >= 2 * H and torch.equal(got, _offline(r.E, rate)[:got.numel()]) and r.stats["comfort"] > 0
